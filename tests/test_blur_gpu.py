"""Gaussian blur on the GPU, through the C ABI (sx_gaussian_blur, sx_gaussian_blur_masked) and through ``gaussian_blur`` /
``GaussianBlurAugment``.

The yardstick is tests/_blur_numpy.py: the rule in float64 on the float32 values the kernel reads, evaluated ONCE per (tile, sigma) and
shared.  Float tiles hold values in [0, 1].  Bounds:
  float outputs          1e-4 on [0, 1], the project's bound for its colour-space maps (TOL of test_hsv_gpu.py), plus half a unit in the
                         last place of the type at 1 for bf16 / f16 outputs: 2^-9 / 2^-12;
  uint8 output           |out - level64| <= 0.5 + 3e-3 levels for EVERY element.  The 3e-3 is derived: two chains of at most 17 fused
                         multiply-adds (33 terms) on values up to 255 give about 1e-3, float32 taps against float64 taps (a 2-ulp expf, a
                         normalising sum of 33 terms) about 1.5e-3;
  uint8 tiles, float out the level is quantised to 8 bits first (the output rule), so the same band holds for 255 x out (x 1 without the
                         / 255), widened by the half unit of the output type where the / 255 is rounded to it.
Copies (sigma NaN, infinite, <= 0 or below 0.125; masked-out pixels) are exact: the output rule applied to the stored element.

The tiles -- 1x1, 1x7, 2x2, 5x3 (axes shorter than the halo: the fold runs several times), 33x31 (odd width, unaligned rows), 64x64
(exactly one block), 65x130 (block seams on both axes, a ragged edge), 144x128 (packs, more than one block row) -- come in batches of 3,
so tiles with different radii sit in one launch.

Measured on an MI355X (the figures this file prints; DESIGN.md 4s quotes them): uint8 output 0.50005 levels, float32 / float64 3.72e-7,
float16 2.443e-4, bfloat16 1.953e-3 (the last two are the rounding of a value to the type), uint8 tiles to bf16 / f16 / float32 0.50005
levels and with ``/ 255`` to bf16 0.99606 and to f16 0.56116 levels; beside a NaN pixel float32 3.0e-7."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import GaussianBlurAugment, _native, focus_statistics, gaussian_blur, tissue_mask
from tests import _blur_numpy as bn
from tests import _focus_numpy as fn
from tests.test_hsv_gpu import graph_nodes, off_by_one

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAND = 0.5 + 3e-3
HALF_ULP_AT_1 = {torch.bfloat16: 2.0**-9, torch.float16: 2.0**-12, torch.float32: 0.0, torch.float64: 0.0}
SHAPES = ((1, 1), (1, 7), (2, 2), (5, 3), (33, 31), (64, 64), (65, 130), (144, 128))
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
NAN, INF = float("nan"), float("inf")
SIGMA_ROWS = ((0.1, 1.0, 4.0), (0.3, 2.5, 7.0), (NAN, 0.0, -1.0), (INF, 0.125, 0.375))
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64)
DTYPE_IDS = [str(d).split(".")[-1] for d in DTYPES]
CL, UNIT = _native.MACENKO_CHANNELS_LAST, _native.MACENKO_NORMALIZE_0_1
OUT_FLAG = {torch.bfloat16: _native.MACENKO_OUT_BF16, torch.float16: _native.MACENKO_OUT_F16}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ the tiles and their references
@lru_cache(maxsize=None)
def tiles_of(dtype: torch.dtype, shape: tuple) -> torch.Tensor:
    """(3, 3, H, W) on the CPU: seeded uint8 levels, or seeded float32 uniforms in [0, 1) rounded to the type (float64 holds them exactly)."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    if dtype == torch.uint8:
        return torch.from_numpy(rng.integers(0, 256, size=(3, 3, *shape), dtype=np.uint8))
    return torch.from_numpy(rng.random((3, 3, *shape), dtype=np.float32)).to(dtype)


@lru_cache(maxsize=None)
def reference(dtype: torch.dtype, shape: tuple, tile: int, sigma: float) -> np.ndarray:
    """(3, H, W) float64: tile ``tile`` of ``tiles_of`` under ``sigma``, before the output rule."""
    out = bn.blur64(bn.input_values(tiles_of(dtype, shape)[tile]), sigma)
    out.setflags(write=False)
    return out


def reference_rows(dtype: torch.dtype, shape: tuple, sigmas) -> np.ndarray:
    return np.stack([reference(dtype, shape, t, float(s)) for t, s in enumerate(sigmas)])


def out_dtype_of(x: torch.Tensor, flags: int) -> torch.dtype:
    if x.dtype == torch.uint8:
        for dtype, flag in OUT_FLAG.items():
            if flags & flag:
                return dtype
        return torch.float32 if flags & UNIT else torch.uint8
    return x.dtype


def raw(lib, x: torch.Tensor, sigmas: torch.Tensor, flags: int = 0, mask: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_gaussian_blur / sx_gaussian_blur_masked on the current stream; ``sigmas``: (R,) float32 on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype_of(x, flags), device=x.device)
    assert sigmas.dtype == torch.float32 and sigmas.is_contiguous() and sigmas.dim() == 1
    stream = _native.stream_ptr(x.device)
    if mask is None:
        rc = lib.sx_gaussian_blur(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, sigmas.data_ptr(), sigmas.shape[0], flags, stream)
    else:
        rc = lib.sx_gaussian_blur_masked(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, sigmas.data_ptr(), sigmas.shape[0], mask.data_ptr(), flags, stream)
    assert rc == 0, _native.last_error(lib)
    return out


def sig(values, dev) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float32, device=dev).reshape(-1)


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def check(out: torch.Tensor, x: torch.Tensor, unit: bool, want: np.ndarray, sigmas, what) -> float:
    """``out``, ``x``: (3, 3, H, W) on the CPU; ``want``: the float64 reference.  Copy tiles are exact; prints the figure, then asserts."""
    in_dtype = x.dtype
    for t, s in enumerate(sigmas):
        if bn.radius(s) == 0:      # a copy: the output rule applied to the stored elements, and the stored elements themselves where nothing converts
            assert torch.equal(out[t], bn.to_output(bn.input_values(x[t]), in_dtype, out.dtype, unit)), (what, t)
            if out.dtype == in_dtype and not unit:
                assert torch.equal(out[t].view(torch.uint8), x[t].view(torch.uint8)), (what, t)
    got = out.to(torch.float64).numpy()
    assert np.isfinite(got).all(), what
    if in_dtype == torch.uint8:
        scale = 255.0 if unit else 1.0
        extra = 0.0 if out.dtype == torch.uint8 or not unit else 255.0 * HALF_ULP_AT_1[out.dtype]
        err = float(np.abs(got * scale - want).max())
        print(f"{what}: max |out - level64| = {err:.5f} levels (band {BAND + extra:.4f})")
        assert err <= BAND + extra, (what, err)
        return err
    assert not unit
    err = float(np.abs(got - want).max())
    bound = TOL + HALF_ULP_AT_1[out.dtype]
    print(f"{what}: max |out - value64| = {err:.3e} on [0, 1] (bound {bound:.3e})")
    assert err <= bound, (what, err)
    return err


# ------------------------------------------------------------------ against the float64 restatement
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_sigma_rows_against_float64(dev, lib, dtype, shape):
    x = tiles_of(dtype, shape)
    xd, xl = x.to(dev), nhwc(x).to(dev)
    for sigmas in SIGMA_ROWS:
        want = reference_rows(dtype, shape, sigmas)
        out = raw(lib, xd, sig(sigmas, dev))
        assert out.dtype == dtype
        check(out.cpu(), x, False, want, sigmas, (str(dtype), shape, sigmas))
        assert torch.equal(raw(lib, xl, sig(sigmas, dev), CL).permute(0, 3, 1, 2), out), (sigmas, "NHWC")      # NCHW and NHWC: the same values
        for t in range(3):      # a tile alone gives the bits it has inside the batch
            assert torch.equal(raw(lib, xd[t:t + 1].contiguous(), sig(sigmas[t:t + 1], dev)), out[t:t + 1]), (sigmas, t)
    # a sigma of 7.0 gives the bits of a sigma of 4.0
    assert torch.equal(raw(lib, xd, sig((7.0, 1e30, 4.5), dev)), raw(lib, xd, sig((4.0,), dev)))
    # one sigma for the batch
    assert torch.equal(raw(lib, xd, sig((2.5,), dev)), raw(lib, xd, sig((2.5, 2.5, 2.5), dev)))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("flags", [OUT_FLAG[torch.bfloat16], OUT_FLAG[torch.float16], UNIT, UNIT | OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16]],
                         ids=["bf16", "f16", "unit_f32", "unit_bf16", "unit_f16"])
def test_uint8_tiles_float_outputs(dev, lib, flags, shape):
    x = tiles_of(torch.uint8, shape)
    xd = x.to(dev)
    for sigmas in SIGMA_ROWS[1::2]:
        want = reference_rows(torch.uint8, shape, sigmas)
        out = raw(lib, xd, sig(sigmas, dev), flags)
        assert out.dtype == out_dtype_of(xd, flags)
        check(out.cpu(), x, bool(flags & UNIT), want, sigmas, (flags, shape, sigmas))
        # the output rule, exactly: the rounded 8-bit level of the plain call, cast -- divided by 255 in float32 and rounded to the type
        level = raw(lib, xd, sig(sigmas, dev)).cpu().to(torch.float32)
        assert torch.equal(out.cpu(), ((level / 255.0) if flags & UNIT else level).to(out.dtype)), (flags, sigmas)
        assert torch.equal(raw(lib, nhwc(xd), sig(sigmas, dev), flags | CL).permute(0, 3, 1, 2), out)


@pytest.mark.parametrize("shape", [(33, 31), (65, 130)], ids=["33x31", "65x130"])
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
def test_normalize_0_1_divides_a_float_tile_by_255(dev, lib, dtype, shape):
    """A float tile's / 255 is the output rule's: the value rounded to the tile's type, divided by 255 in float32 (float64 tiles: in
    float64), rounded to the type again -- an exact relation to the call without the flag, copies included."""
    xd = (tiles_of(dtype, shape).to(torch.float32) * 255.0).to(dtype).to(dev)      # (levels: what the flag is for)
    sigmas = sig((0.0, 1.0, 4.0), dev)
    value, unit = raw(lib, xd, sigmas).cpu(), raw(lib, xd, sigmas, UNIT).cpu()
    want = value / 255.0 if dtype == torch.float64 else (value.to(torch.float32) / 255.0).to(dtype)
    assert torch.equal(unit, want), (dtype, shape)


# ------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_constant_tile_stays_constant(dev, lib, dtype):
    for shape in ((5, 3), (65, 130)):
        levels = torch.tensor([0, 37, 200, 255, 1, 128, 254, 77, 13], dtype=torch.float32).reshape(3, 3, 1, 1).expand(3, 3, *shape)
        x = (levels.to(torch.uint8) if dtype == torch.uint8 else (levels / 255.0).to(dtype)).contiguous().to(dev)
        for sigmas in SIGMA_ROWS + ((0.5, 2.0, 3.3),):
            out = raw(lib, x, sig(sigmas, dev))
            assert bool((out == out[:, :, :1, :1]).all()), (dtype, shape, sigmas)      # constant, every plane
            if dtype == torch.uint8:
                assert torch.equal(out, x), (shape, sigmas)      # and the very level: rounded to nearest
            else:      # the taps sum to 1 within float32: per pass at most 18 roundings in the taps' sum and 17 in the chain, each 2^-24 at 1
                err = float((out.double() - x.double()).abs().max())
                assert err <= 2 * 35 * 2.0**-24 + HALF_ULP_AT_1[dtype], (dtype, shape, sigmas, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_pointers_one_element_off_give_the_aligned_bits(dev, lib, dtype):
    shape = (144, 128)
    x = tiles_of(dtype, shape).to(dev)
    sigmas = sig((0.0, 1.0, 4.0), dev)
    mask = (torch.rand(3, *shape, device=dev) < 0.7).to(torch.uint8)
    want, want_masked = raw(lib, x, sigmas), raw(lib, x, sigmas, mask=mask)
    assert torch.equal(raw(lib, off_by_one(x), sigmas), want)
    out = off_by_one(torch.empty_like(want))
    assert torch.equal(raw(lib, x, sigmas, out=out), want)
    assert torch.equal(raw(lib, x, sigmas, mask=off_by_one(mask)), want_masked)
    assert torch.equal(raw(lib, off_by_one(x), sigmas, mask=mask), want_masked)
    assert torch.equal(raw(lib, off_by_one(nhwc(x)), sigmas, CL).permute(0, 3, 1, 2), want)


def test_float_copies_keep_nan_payloads_and_negative_zero(dev, lib):
    bits = torch.tensor([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], dtype=torch.int64).to(torch.int32)
    x = bits.view(torch.float32).repeat(3 * 3 * 5 * 7 // 7).reshape(3, 3, 5, 7).contiguous().to(dev)
    for sigmas in ((NAN, 0.0, -1.0), (INF, 0.1, -INF)):
        assert torch.equal(raw(lib, x, sig(sigmas, dev)).view(torch.int32), x.view(torch.int32))
    half = x.to(torch.float16)
    assert torch.equal(raw(lib, half, sig((0.0,), dev)).view(torch.int16), half.view(torch.int16))


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("shape", [(5, 3), (33, 31), (65, 130), (144, 128)], ids=["5x3", "33x31", "65x130", "144x128"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_masks(dev, lib, dtype, shape):
    x = tiles_of(dtype, shape).to(dev)
    sigmas = sig((0.7, 2.0, 4.0), dev)
    plain = raw(lib, x, sigmas)
    copied = raw(lib, x, sig((NAN,), dev))
    if dtype != torch.float64:      # (a float64 tile is read as float32: its copy holds the float32 values, which these tiles hold already)
        assert torch.equal(copied.view(torch.uint8), x.view(torch.uint8))
    assert torch.equal(copied, x)
    assert torch.equal(raw(lib, x, sigmas, mask=torch.ones(3, *shape, dtype=torch.uint8, device=dev)), plain)
    assert torch.equal(raw(lib, x, sigmas, mask=torch.zeros(3, *shape, dtype=torch.uint8, device=dev)), x)
    mask = (torch.rand(3, *shape, device=dev) < 0.6).to(torch.uint8) * 255      # (non-zero = in)
    got = raw(lib, x, sigmas, mask=mask)
    inside = mask.bool().unsqueeze(1).expand_as(x)
    assert torch.equal(got[~inside], x[~inside]) and torch.equal(got[inside], plain[inside])      # out: the input's bits; in: the unmasked call's bits
    assert not torch.equal(got, plain)
    for flags in ((UNIT,) if dtype != torch.uint8 else (UNIT, OUT_FLAG[torch.bfloat16])):
        assert torch.equal(raw(lib, x, sigmas, flags, mask=mask), torch.where(inside, raw(lib, x, sigmas, flags), raw(lib, x, sig((NAN,), dev), flags)))


def test_luminosity_rule_is_the_explicit_tissue_mask(dev):
    x = torch.from_numpy(fn.real_crop(128, 128, 3).copy()).to(dev)      # (the shared crop is read-only)
    sigmas = sig((1.0, 2.0, 3.0), dev)
    explicit, counts = tissue_mask(x, 0.7)
    assert 0 < int(counts.sum()) < explicit.numel()
    want = gaussian_blur(x, sigmas, mask=explicit)
    assert torch.equal(gaussian_blur(x, sigmas, mask="luminosity", luminosity_threshold=0.7), want)
    assert torch.equal(GaussianBlurAugment(mask="luminosity", luminosity_threshold=0.7, normalize_to_0_1=False)(x, sigmas), want)
    assert torch.equal(GaussianBlurAugment(normalize_to_0_1=False)(x, sigmas, mask=explicit.unsqueeze(1)), want)
    assert not torch.equal(want, gaussian_blur(x, sigmas))


# ------------------------------------------------------------------ non-finite pixels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_a_nan_pixel_spreads_over_its_window_and_no_further(dev, lib, dtype):
    shape, place = (65, 130), (1, 60, 66)      # (channel, row, column): next to the block seams
    x = tiles_of(dtype, shape).clone()
    x[:, place[0], place[1], place[2]] = NAN
    sigmas = (0.5, 1.0, 4.0)
    out = raw(lib, x.to(dev), sig(sigmas, dev)).cpu()
    rows, cols = torch.arange(shape[0]).reshape(-1, 1), torch.arange(shape[1]).reshape(1, -1)
    for t, s in enumerate(sigmas):
        r = bn.radius(s)
        window = ((rows - place[1]).abs() <= r) & ((cols - place[2]).abs() <= r)      # (the fold at the bottom border lands on rows the window holds already)
        expect = torch.zeros(3, *shape, dtype=torch.bool)
        expect[place[0]] = window
        assert torch.equal(torch.isnan(out[t]), expect), (dtype, s)
        clean = tiles_of(dtype, shape)[t]
        want = torch.from_numpy(bn.blur64(bn.input_values(clean), s))
        err = float((out[t].double() - want)[~expect].abs().max())
        print(f"NaN pixel, {dtype}, sigma {s}: max |out - value64| outside the window = {err:.3e}")
        assert err <= TOL + HALF_ULP_AT_1[dtype], (dtype, s, err)


# ------------------------------------------------------------------ the module and the functional form
def test_module_and_functional_form(dev, lib):
    x = tiles_of(torch.uint8, (65, 130)).to(dev)
    sigmas = sig((0.3, 2.5, 7.0), dev)
    want = raw(lib, x, sigmas)
    assert torch.equal(gaussian_blur(x, sigmas), want)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        gaussian_blur(x.cpu(), sigmas)
    aug = GaussianBlurAugment(normalize_to_0_1=False)
    assert torch.equal(aug(x, sigmas), want) and torch.equal(aug(x, sigmas.cpu()), want)
    assert torch.equal(GaussianBlurAugment()(x, sigmas), raw(lib, x, sigmas, UNIT))      # normalize_to_0_1 defaults to True, as HSVAugment's
    assert torch.equal(gaussian_blur(x, sigmas, out_dtype=torch.bfloat16), raw(lib, x, sigmas, OUT_FLAG[torch.bfloat16]))
    assert torch.equal(gaussian_blur(nhwc(x), sigmas, channel_axis=-1), nhwc(want))
    # one sigma for the batch: a (1,) row, a () tensor, a Python number
    one = raw(lib, x, sig((2.5,), dev))
    assert torch.equal(gaussian_blur(x, sigmas[1:2]), one) and torch.equal(gaussian_blur(x, sigmas[1]), one) and torch.equal(gaussian_blur(x, 2.5), one) and torch.equal(aug(x, 2.5), one)
    assert torch.equal(gaussian_blur(x, 0), x) and torch.equal(gaussian_blur(x, 0.1), x) and torch.equal(gaussian_blur(x, 4), raw(lib, x, sig((4.0,), dev)))
    # CHW in, CHW out
    single = aug(x[1], sigmas[1:2])
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, want[1])
    assert torch.equal(gaussian_blur(x[1], 2.5), want[1])
    # p = 0: every sigma is NaN, the input comes back exactly; sigma = (0, 0): the same
    assert torch.equal(GaussianBlurAugment(p=0.0, normalize_to_0_1=False)(x), x)
    assert torch.equal(GaussianBlurAugment((0.0, 0.0), normalize_to_0_1=False)(x), x)
    # a draw: the sigmas sample_rows gives with the same seed, on the device when the generator is there
    for where in ("cpu", dev):
        drawn = GaussianBlurAugment((0.0, 4.0), p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5))
        got = drawn(x)
        again = GaussianBlurAugment((0.0, 4.0), p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5)).sample_rows(3, dev)
        assert torch.equal(got, raw(lib, x, again.contiguous()))
        left = torch.isnan(again)
        assert torch.equal(got[left], x[left])


# ------------------------------------------------------------------ capture
def test_a_captured_forward_replays_with_new_sigmas_and_images(dev):
    first_x, second_x = tiles_of(torch.uint8, (65, 130)).to(dev), tiles_of(torch.uint8, (65, 130)).flip(0).contiguous().to(dev)
    first, second = sig((0.3, 2.5, 7.0), dev), sig((1.0, NAN, 0.6), dev)
    aug = GaussianBlurAugment(normalize_to_0_1=False)
    want_first, want_second = aug(first_x, first), aug(second_x, second)
    assert not torch.equal(want_first, want_second)
    x, buf = first_x.clone(), first.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        aug(x, buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = aug(x, buf)
        types, roots, edges = graph_nodes(dev)
    assert types == [0], types      # ONE node, a kernel (hipGraphNodeTypeKernel = 0): no memset node (2), no copy (1)
    assert roots == 1 and edges == 0      # a single branch
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_first)
    buf.copy_(second)
    x.copy_(second_x)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_second)


# ------------------------------------------------------------------ with the focus measurement
FOCUS_SIGMAS = (0.0, 0.5, 1.0, 2.0, 4.0)


def test_blur_lowers_the_laplacian_variance_of_real_tissue(dev):
    """A convex smoothing cannot raise the Laplacian energy of natural tissue: the Laplacian variance of a real 128 x 128 crop strictly
    decreases over sigma = 0 (the copy), 0.5, 1, 2, 4 -- in the two CPU restatements first (the crop satisfies the condition), then on the
    device, where ``focus_statistics`` of the blurred tiles also equals the restatement's integers on the device's own output."""
    crop = fn.real_crop(128, 128, 1)      # (1, 3, 128, 128) uint8
    cpu = []
    for s in FOCUS_SIGMAS:
        blurred = bn.to_output(bn.blur64(crop[0].astype(np.float64), s), torch.uint8, torch.uint8, False).numpy()[None]
        pixels, sums, squares, _ = (int(v.reshape(-1)[0]) for v in fn.statistics(blurred))
        cpu.append(float(fn.variance_exact(pixels, sums, squares)))
    print("Laplacian variance over sigma", FOCUS_SIGMAS, "restatements:", [f"{v:.3f}" for v in cpu])
    assert all(a > b for a, b in zip(cpu, cpu[1:])), cpu
    x = torch.from_numpy(crop.copy()).to(dev).expand(len(FOCUS_SIGMAS), -1, -1, -1).contiguous()
    out = gaussian_blur(x, sig(FOCUS_SIGMAS, dev))
    assert torch.equal(out[0], x[0])
    stats = focus_statistics(out)
    got = stats.laplacian_variance().reshape(-1).cpu().tolist()
    print("Laplacian variance over sigma", FOCUS_SIGMAS, "device:", [f"{v:.3f}" for v in got])
    assert all(a > b for a, b in zip(got, got[1:])), got
    assert np.array_equal(torch.stack([w.reshape(-1) for w in stats]).cpu().numpy(), fn.statistics(out.cpu().numpy()).reshape(4, -1))


# ------------------------------------------------------------------ the C ABI's refusals leave the output alone
def test_argument_errors_launch_nothing(dev, lib):
    x = tiles_of(torch.uint8, (33, 31)).to(dev)
    out = torch.full_like(x, 7)
    sigmas, mask = sig((1.0, 2.0, 3.0), dev), torch.ones(3, 33, 31, dtype=torch.uint8, device=dev)
    code, stream, bad = _native.DTYPE_CODES[torch.uint8], _native.stream_ptr(dev), _native.SX_ERR_BAD_ARG
    p = lambda t: t.data_ptr()      # noqa: E731
    assert lib.sx_gaussian_blur(None, p(out), code, 3, 33, 31, p(sigmas), 3, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), None, code, 3, 33, 31, p(sigmas), 3, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), p(out), code, 3, 33, 31, None, 3, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), p(out), code, 3, -33, 31, p(sigmas), 3, 0, stream) == bad and "positive" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), p(out), code, -3, 33, 31, p(sigmas), 3, 0, stream) == bad and "positive" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), p(out), code, 3, 33, 31, p(sigmas), 2, 0, stream) == bad and "n_rows" in _native.last_error(lib)
    assert lib.sx_gaussian_blur_masked(p(x), p(out), code, 3, 33, 31, p(sigmas), 3, None, 0, stream) == bad and "mask pointer is null" in _native.last_error(lib)
    assert lib.sx_gaussian_blur_masked(p(x), p(out), code, 3, 33, 31, p(sigmas), 3, p(mask), CL, stream) == bad and "planar" in _native.last_error(lib)
    assert lib.sx_gaussian_blur(p(x), p(out), 17, 3, 33, 31, p(sigmas), 3, 0, stream) == _native.SX_ERR_DTYPE
    torch.cuda.synchronize(dev)
    assert bool((out == 7).all())
