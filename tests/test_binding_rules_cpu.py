"""The binding's shape and dtype rules (stainx_amd/backends/torch_hip_backend.py) on CPU tensors: what each accepts and returns, and the
full text of every refusal.  The messages are the ones the methods raised when every method spelt its own checks out: a rule that is
written once must not change what a caller reads."""
import pytest
import torch

from stainx_amd.backends import torch_hip_backend as be

U8, F16, BF16, F32, F64 = torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64
NORM, NHWC, OUT_BF16, OUT_F16 = 1, 2, 32, 64      # include/stainx_hip.h: SX_MACENKO_*
CPU = torch.device("cpu")


def z(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype)


def refused(kind, message, rule, *args):
    with pytest.raises(kind) as caught:
        rule(*args)
    assert str(caught.value) == message, (rule.__name__, args)


def test_out_dtype_rule():
    for dtype in (U8, F16, BF16, F32, F64):
        images = z(2, 3, 4, 5, dtype=dtype)
        for out_dtype in (None, dtype, BF16, F16, F32):
            for norm in (False, True):
                for last in (False, True):
                    base = (NORM if norm else 0) | (NHWC if last else 0)
                    if out_dtype is None or out_dtype == dtype:
                        assert be._out_flags(images, out_dtype, norm, last) == (base, F32 if (norm and dtype == U8) else dtype)
                    elif dtype == U8 and out_dtype in (BF16, F16):
                        assert be._out_flags(images, out_dtype, norm, last) == (base | (OUT_BF16 if out_dtype == BF16 else OUT_F16), out_dtype)
                    else:
                        refused(ValueError, f"out_dtype is supported for uint8 input and bfloat16 / float16 output, got {dtype} -> {out_dtype}",
                                be._out_flags, images, out_dtype, norm, last)
    refused(ValueError, "out_dtype is supported for uint8 input and bfloat16 / float16 output, got torch.uint8 -> torch.float32", be._out_flags, z(1, 3, 2, 2, dtype=U8), F32, True, False)
    refused(ValueError, "out_dtype is supported for uint8 input and bfloat16 / float16 output, got torch.float32 -> torch.bfloat16", be._out_flags, z(1, 3, 2, 2), BF16, False, False)


def test_dtype_code():
    assert [be._dtype_code(z(1, dtype=d)) for d in (U8, F16, BF16, F32, F64)] == [0, 1, 2, 3, 4]
    refused(TypeError, "unsupported image dtype torch.int32; supported: ['torch.bfloat16', 'torch.float16', 'torch.float32', 'torch.float64', 'torch.uint8']",
            be._dtype_code, z(1, dtype=torch.int32))


def test_image_shapes():
    assert be._image_shape(z(2, 3, 4, 5), False, "Macenko", "transform") == (2, 4, 5)
    assert be._image_shape(z(2, 4, 5, 3), True, "Macenko", "transform") == (2, 4, 5)
    assert be._image_shape(z(0, 3, 4, 5), False, "Reinhard") == (0, 4, 5) and be._image_shape(z(2, 3, 0, 5), False, "deconvolution", "apply") == (2, 0, 5)
    assert be._image_shape(z(2, 4, 5, 3), True, "HistogramMatching") == (2, 4, 5) and be._image_shape(z(2, 3, 4, 5), False, "Macenko fit") == (2, 4, 5)
    assert be._image_shape(z(2, 1, 4, 5), False, None) == (2, 4, 5)      # (the mask / level functions: their callers have checked)
    for rule_args, message in (
        ((z(3, 4, 5), False, "Macenko", "transform"), "Macenko expects NCHW images, got shape (3, 4, 5)"),
        ((z(2, 4, 5, 3), False, "Macenko", "augment"), "Macenko augment expects 3 channels in dim 1 (NCHW), got C=4 with shape (2, 4, 5, 3)"),
        ((z(2, 3, 4, 5), True, "Macenko", "separate"), "Macenko separate with channels_last expects NHWC images with C=3, got shape (2, 3, 4, 5)"),
        ((z(4, 5, 3), True, "Macenko", "estimate"), "Macenko estimate with channels_last expects NHWC images with C=3, got shape (4, 5, 3)"),
        ((z(2, 1, 4, 5), False, "Macenko fit"), "Macenko fit expects NCHW with C=3, got shape (2, 1, 4, 5)"),
        ((z(2, 4, 5, 3), False, "deconvolution", "apply"), "deconvolution apply expects NCHW tensors with 3 channels, got shape (2, 4, 5, 3)"),
        ((z(2, 3, 4, 5), True, "deconvolution", "quantify"), "deconvolution quantify expects NHWC tensors with 3 channels, got shape (2, 3, 4, 5)"),
        ((z(3, 4, 5), False, "deconvolution", "combine"), "deconvolution combine expects NCHW tensors with 3 channels, got shape (3, 4, 5)"),
        ((z(2, 4, 5, 3), False, "Reinhard"), "Reinhard expects NCHW images with C=3, got shape (2, 4, 5, 3)"),
        ((z(3, 4, 5), False, "Reinhard"), "Reinhard expects NCHW images with C=3, got shape (3, 4, 5)"),
        ((z(3, 4, 5), False, "HistogramMatching"), "HistogramMatching expects 4D images, got shape (3, 4, 5)"),
        ((z(3, 4, 5), True, "HistogramMatching"), "HistogramMatching expects 4D images, got shape (3, 4, 5)"),
        ((z(2, 4, 5, 3), False, "HistogramMatching"), "HistogramMatching expects 3 channels, got 4 with shape (2, 4, 5, 3)"),
        ((z(2, 3, 4, 5), True, "HistogramMatching"), "HistogramMatching expects 3 channels, got 5 with shape (2, 3, 4, 5)"),
    ):
        refused(ValueError, message, be._image_shape, *rule_args)


def test_reference_pair():
    assert be._reference_pair(z(3, 2), z(2)) is True and be._reference_pair(z(3, 2), z(1, 2), "both or neither") is True
    assert be._reference_pair(None, None, "both or neither") is False
    refused(ValueError, "stain_matrix must have shape (3, 2), got torch.Size([2, 3])", be._reference_pair, z(2, 3), z(2))
    refused(ValueError, "stain_matrix must have shape (3, 2), got torch.Size([1, 3, 2])", be._reference_pair, z(1, 3, 2), z(2), "x")
    refused(ValueError, "target_max_conc must have 2 elements, got 3", be._reference_pair, z(3, 2), z(3))
    refused(ValueError, "target_max_conc must have 2 elements, got 4", be._reference_pair, z(3, 2), z(2, 2), "x")
    for together in ("both (normalise and jitter) or neither (each tile's own stain basis)",      # augment, augment_masked
                     "both (normalised) or neither (each tile's own stain basis)",                   # separate
                     "both (normalise) or neither (the given source basis is kept)",                 # apply, apply_masked
                     "both (normalised) or neither (the source basis itself)"):                      # separate_apply, separate_apply_masked, separate_masked
        refused(ValueError, f"stain_matrix and target_max_conc go together: {together}", be._reference_pair, z(3, 2), None, together)
        refused(ValueError, f"stain_matrix and target_max_conc go together: {together}", be._reference_pair, None, z(2), together)


def test_source_basis():
    for n in (1, 2, 3):
        assert be._source_rows(z(3, 2), z(2), n, True) == 1 and be._source_rows(z(3, 2), z(1, 2), n, True) == 1
        assert be._source_rows(z(1, 3, 2), z(2), n, True) == 1 and be._source_rows(z(1, 3, 2), None, n, False) == 1
        assert be._source_rows(z(n, 3, 2), z(n, 2), n, True) == n and be._source_rows(z(n, 3, 2), z(2 * n), n, False) == n
        for wrong in (z(2, 3), z(3, 3), z(n + 1, 3, 2), z(n, 2, 3), z(1, 1, 3, 2), z(6)):
            refused(ValueError, f"source_he must have shape (3, 2), (1, 3, 2) or (N, 3, 2) = ({n}, 3, 2), got {tuple(wrong.shape)}", be._source_rows, wrong, z(2), n, True)
        for wrong in (z(3), z(2, n + 1), z(n + 1, 2), z(1, n, 2)):
            refused(ValueError, f"source_max_c must hold 2 values per source basis, ({n}, 2), got shape {tuple(wrong.shape)}", be._source_rows, z(n, 3, 2), wrong, n, True)
        refused(ValueError, "source_max_c must hold 2 values per source basis, (1, 2), got shape (2, 1)", be._source_rows, z(3, 2), z(2, 1), n, False)
        refused(ValueError, "source_max_c is required to normalise to a reference (it may be None in own-basis mode only)", be._source_rows, z(n, 3, 2), None, n, True)


def test_factors():
    assert be._check_factors(z(4, 2), z(4, 2), 4, 2) is None and be._check_factors(z(1, 3), z(1, 3), 1, 3) is None and be._check_factors(z(0, 2), z(0, 2), 0, 2) is None
    refused(ValueError, "alpha and beta must have shape (N, 2) = (4, 2), got (4, 3) and (4, 2)", be._check_factors, z(4, 3), z(4, 2), 4, 2)
    refused(ValueError, "alpha and beta must have shape (N, 2) = (4, 2), got (4, 2) and (2,)", be._check_factors, z(4, 2), z(2), 4, 2)
    refused(ValueError, "alpha and beta must have shape (N, 2) = (4, 2), got (1, 2) and (1, 2)", be._check_factors, z(1, 2), z(1, 2), 4, 2)
    refused(ValueError, "alpha and beta must have shape (N, 3) = (2, 3), got (2, 2) and (2, 2)", be._check_factors, z(2, 2), z(2, 2), 2, 3)
    refused(ValueError, "alpha and beta must have shape (N, 3) = (2, 3), got (3,) and (2, 3)", be._check_factors, z(3), z(2, 3), 2, 3)


def test_statistics_rows():
    for accepted in ("(3,), (1, 3)", "(1, 3)"):      # apply_targets[_masked] / apply_statistics[_masked]: each call keeps its wording
        for n in (1, 4):
            for mean, std, rows in ((z(3), z(3), 1), (z(1, 3), z(3), 1), (z(n, 3), z(n, 3), n)):
                got = be._statistics_rows(mean, std, n, "source", accepted)
                assert tuple(got[0].shape) == (rows, 3) and tuple(got[1].shape) == (rows, 3)
        refused(ValueError, f"source_mean must be {accepted} or (4, 3) for 4 tiles, got shape (2, 3)", be._statistics_rows, z(2, 3), z(4, 3), 4, "source", accepted)
        refused(ValueError, f"source_std must be {accepted} or (4, 3) for 4 tiles, got shape (1, 4)", be._statistics_rows, z(3), z(4), 4, "source", accepted)
        refused(ValueError, f"target_mean must be {accepted} or (4, 3) for 4 tiles, got shape (4, 1, 3)", be._statistics_rows, z(4, 1, 3), z(4, 3), 4, "target", accepted)
        refused(ValueError, "source_mean and source_std must have the same number of rows, got 1 and 4", be._statistics_rows, z(3), z(4, 3), 4, "source", accepted)
    refused(ValueError, "target_std must be (3,), (1, 3) or (2, 3) for 2 tiles, got shape (3, 3)", be._statistics_rows, z(3), z(3, 3), 2, "target")
    assert be._reference_statistics(z(3), z(1, 3)) is None and be._reference_statistics(z(3, 1), z(1, 1, 3)) is None
    for mean, std in ((z(2), z(3)), (z(3), z(4)), (z(2, 3), z(3))):
        refused(ValueError, "reference_mean / reference_std must have 3 elements", be._reference_statistics, mean, std)


def test_bases():
    for n in (1, 2, 5):
        assert be._basis_rows(z(3, 3), n, "basis") == 1 and be._basis_rows(z(1, 3, 3), n, "target") == 1 and be._basis_rows(z(n, 3, 3), n, "basis") == n
        for what in ("basis", "target"):
            for wrong in (z(3, 2), z(9), z(n + 1, 3, 3), z(n, 3, 2), z(1, 1, 3, 3)):
                refused(ValueError, f"{what} must have shape (3, 3), (1, 3, 3) or (N, 3, 3) = ({n}, 3, 3), got {tuple(wrong.shape)}", be._basis_rows, wrong, n, what)


def test_explicit_mask():
    good = torch.ones(2, 4, 5, dtype=U8)
    assert be._explicit_mask(good, 2, 4, 5, CPU) is good      # (dense uint8 on the device already: the tensor itself)
    as_bool = torch.ones(2, 4, 5, dtype=torch.bool)
    got = be._explicit_mask(as_bool, 2, 4, 5, CPU)
    assert got.dtype == U8 and tuple(got.shape) == (2, 4, 5) and got.data_ptr() == as_bool.data_ptr()      # (bool: the same bytes)
    got = be._explicit_mask(torch.ones(2, 1, 4, 5, dtype=torch.bool), 2, 4, 5, CPU)
    assert got.dtype == U8 and tuple(got.shape) == (2, 4, 5) and got.is_contiguous()
    assert be._mask_bytes(None, CPU) is None
    refused(ValueError, "mask must be uint8 / bool (N, H, W) = (2, 4, 5), got torch.uint8 (2, 5, 4)", be._explicit_mask, torch.ones(2, 5, 4, dtype=U8), 2, 4, 5, CPU)
    refused(ValueError, "mask must be uint8 / bool (N, H, W) = (2, 4, 5), got torch.uint8 (1, 4, 5)", be._explicit_mask, torch.ones(1, 4, 5, dtype=torch.bool), 2, 4, 5, CPU)
    refused(ValueError, "mask must be uint8 / bool (N, H, W) = (2, 4, 5), got torch.uint8 (4, 5)", be._explicit_mask, torch.ones(4, 5, dtype=U8), 2, 4, 5, CPU)
    refused(ValueError, "mask must be uint8 / bool (N, H, W) = (2, 4, 5), got torch.float32 (2, 4, 5)", be._explicit_mask, torch.ones(2, 4, 5), 2, 4, 5, CPU)
    refused(ValueError, "mask must be uint8 / bool (N, H, W) = (2, 4, 5), got torch.int64 (2, 4, 5)", be._explicit_mask, torch.ones(2, 4, 5, dtype=torch.int64), 2, 4, 5, CPU)
