"""Gaussian blur without a GPU: the two entry points are declared and exported, their argument errors at the C ABI return before anything
is enqueued, the float64 restatement of the rule (tests/_blur_numpy.py) is held to ``scipy.ndimage.gaussian_filter(mode="mirror",
truncate=4.0)``, the radius rule is held at its boundaries in float32, and ``gaussian_blur`` / ``GaussianBlurAugment`` validate and draw what
they say."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import GaussianBlurAugment, _native, gaussian_blur
from tests import _blur_numpy as bn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_gaussian_blur": 10, "sx_gaussian_blur_masked": 11}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
SCIPY_TOL = 1e-9      # two float64 evaluations of the same sums (measured: 1.2e-13)
SHAPES = ((1, 1), (1, 7), (2, 2), (5, 3), (33, 31), (65, 130))
SIGMAS = (0.1, 0.125, 0.3, 1.0, 2.5, 4.0)


def test_declared_exported_and_public():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert f"#define SX_BLUR_MAX_SIGMA {bn.MAX_SIGMA}f" in header and stainx_amd.blur.MAX_SIGMA == bn.MAX_SIGMA
    for name in ("GaussianBlurAugment", "gaussian_blur"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.blur, name)
    assert isinstance(GaussianBlurAugment(), torch.nn.Module) and callable(gaussian_blur)
    assert "kBlurMaxSigma = 4.0f" in (ROOT / "stainx_amd" / "csrc" / "blur.hpp").read_text()


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, sigmas=FAKE, n_rows=3, flags=0):
        return lib.sx_gaussian_blur(images, out, dtype, n, h, w, sigmas, n_rows, flags, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, sigmas=FAKE, n_rows=3, mask=FAKE, flags=0):
        return lib.sx_gaussian_blur_masked(images, out, dtype, n, h, w, sigmas, n_rows, mask, flags, None)

    for fn in (call, masked):
        for name in ("images", "out", "sigmas"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        for size in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": -1}):
            assert fn(**size) == BAD and "positive" in _native.last_error(lib), size
        assert fn(n=1 << 20, h=1 << 10, w=1 << 10, n_rows=1) == BAD and "2^32" in _native.last_error(lib)
        for rows in (0, 2, 4, -1):
            assert fn(n_rows=rows) == BAD and "n_rows" in _native.last_error(lib), rows
        for flags in (_native.MACENKO_SAMPLED, 1 << 20, _native.MACENKO_TWO_PASS, bf16, f16):      # (the output flags: uint8 input only)
            assert fn(flags=flags) == BAD, flags
        assert fn(dtype=u8, flags=bf16 | f16) == BAD      # (one of the two)
        assert fn(dtype=17) == DTYPE and fn(dtype=17, n_rows=1, flags=classic | unit) == DTYPE and fn(dtype=-1) == DTYPE
    assert call(dtype=99, flags=cl) == DTYPE      # (the unmasked call takes the layout flag; nothing is enqueued for an unknown element type)
    assert masked(mask=None) == BAD and "mask pointer is null" in _native.last_error(lib)
    assert masked(flags=cl) == BAD and "planar" in _native.last_error(lib)
    assert masked(flags=cl, dtype=17) == BAD      # (the argument errors come before the dtype)


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_restatement_agrees_with_scipy(shape):
    from scipy import ndimage

    rng = np.random.default_rng(11 + shape[0] * 131 + shape[1])
    planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
    for sigma in SIGMAS:
        got = bn.blur64(planes, sigma)
        if bn.radius(sigma) == 0:
            assert np.array_equal(got, planes), sigma      # (a copy; scipy's radius there is 0 as well: int(4 * 0.1 + 0.5))
        s = float(np.float32(sigma))
        want = np.stack([ndimage.gaussian_filter(p, s, mode="mirror", truncate=4.0) for p in planes])
        err = float(np.abs(got - want).max())
        print(f"restatement against scipy, {shape}, sigma {sigma}: max |diff| {err:.3e} levels")
        assert err <= SCIPY_TOL, (shape, sigma, err)
        assert got.min() >= planes.min() - 1e-9 and got.max() <= planes.max() + 1e-9      # a convex combination


def test_fold_reflects_without_repeating_the_edge_as_often_as_needed():
    assert bn.fold(np.arange(-17, 18), 1).tolist() == [0] * 35
    assert bn.fold(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert bn.fold(np.arange(-5, 9), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    n = 7
    padded = np.pad(np.arange(n), 16, mode="reflect")      # numpy folds as often as needed, too
    assert bn.fold(np.arange(-16, n + 16), n).tolist() == padded.tolist()


def test_radius_rule_at_its_boundaries_in_float32():
    # (float32 sigmas; the sum 4 sigma + 0.5 is exact: rounded to float32 it would tie up to 1.0 for the float just below 0.125)
    below = lambda v: np.nextafter(np.float32(v), np.float32(0))      # noqa: E731
    assert bn.radius(0.125) == 1 and bn.radius(below(0.125)) == 0
    assert bn.radius(0.375) == 2 and bn.radius(below(0.375)) == 1
    assert bn.radius(4.0) == 16 and bn.radius(7.0) == 16 and bn.radius(3.875) == 16 and bn.radius(below(3.875)) == 15
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), 0.1):
        assert bn.radius(bad) == 0, bad
    assert np.array_equal(bn.taps(7.0), bn.taps(4.0)) and len(bn.taps(4.0)) == 33 and len(bn.taps(0.125)) == 3
    for sigma in SIGMAS[1:]:
        w = bn.taps(sigma)
        assert abs(w.sum() - 1.0) <= 1e-15 and (w > 0).all() and np.array_equal(w, w[::-1])


def test_float32_restatement_stays_close_to_float64():
    """The rule in numpy float32 (taps, both passes) stays within 1e-3 levels of float64 (printed; measured 8.5e-5): the uint8 band's
    3e-3 levels of slack is well above it."""
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 256, size=(3, 65, 130)).astype(np.float64)
    for sigma in SIGMAS[1:]:
        r, s = bn.radius(sigma), np.float32(sigma)
        i = np.arange(-r, r + 1, dtype=np.float32)
        w = np.exp(-(i * i) / (np.float32(2.0) * s * s)).astype(np.float32)
        w = w / w.sum(dtype=np.float32)
        got = bn.filter_axis(bn.filter_axis(planes.astype(np.float32), w, -1), w, -2)
        assert got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - bn.blur64(planes, sigma)).max())
        print(f"float32 restatement against float64, sigma {sigma}: max |diff| {err:.3e} levels")
        assert err <= 1e-3, (sigma, err)


def test_output_rule_rounds_uint8_levels_to_nearest():
    value = np.array([0.0, 0.49, 0.5, 1.5, 2.5, 199.99998, 254.51, 255.0])
    assert bn.to_output(value, torch.uint8, torch.uint8, False).tolist() == [0, 0, 0, 2, 2, 200, 255, 255]
    assert torch.equal(bn.to_output(value, torch.uint8, torch.float32, True), torch.tensor([0, 0, 0, 2, 2, 200, 255, 255], dtype=torch.float32) / 255.0)
    assert bn.to_output(value, torch.uint8, torch.bfloat16, False).dtype == torch.bfloat16
    assert torch.equal(bn.to_output(value, torch.float32, torch.float32, False), torch.from_numpy(value).float())


# ------------------------------------------------------------------ the module and the functional form
def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"sigma": 1.0}, "pair"), ({"sigma": (1.0,)}, "pair"), ({"sigma": (1.0, 2.0, 3.0)}, "pair"), ({"sigma": (-0.1, 1.0)}, "sigma lo"),
                         ({"sigma": (0.0, 4.1)}, "sigma hi"), ({"sigma": (float("nan"), 1.0)}, "sigma lo"), ({"sigma": (0.0, float("inf"))}, "sigma hi"),
                         ({"sigma": ("a", 1.0)}, "sigma lo must be a number"), ({"sigma": (2.0, 1.0)}, "lo <= hi"), ({"p": 1.5}, "p must"), ({"p": -0.1}, "p must"),
                         ({"p": float("nan")}, "p must"), ({"mask": "otsu"}, "mask must be"), ({"luminosity_threshold": 1.5}, "luminosity_threshold"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            GaussianBlurAugment(**kwargs)
    aug = GaussianBlurAugment((0.0, 4.0), p=0.0)      # the closed ends
    assert aug.sigma == (0.0, 4.0) and aug.p == 0.0 and GaussianBlurAugment().sigma == (0.1, 2.0) and GaussianBlurAugment([1, 1]).sigma == (1.0, 1.0)
    assert "sigma=(0.0, 4.0)" in repr(aug) and "p=0.0" in repr(aug) and "normalize_to_0_1=True" in repr(aug) and "mask=None" in repr(aug)
    assert "'luminosity' (luminosity_threshold=0.7)" in repr(GaussianBlurAugment(mask="luminosity", luminosity_threshold=0.7))


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    sigmas = torch.ones(4)
    aug = GaussianBlurAugment()
    for fn in (lambda *a, **k: gaussian_blur(*a, **k), lambda img, r, **k: aug(img, r, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), sigmas)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), sigmas)
        for wrong in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(1, 4), torch.zeros(2)):
            with pytest.raises(ValueError, match=r"sigma must be a number or a tensor of shape \(\), \(1,\) or \(N,\) = \(4,\)"):
                fn(x, wrong)
        for wrong in (-0.5, 4.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=r"sigma must be finite and lie in \[0, 4.0\]"):
                fn(x, wrong)
        for wrong in ("wide", [1.0, 2.0]):
            with pytest.raises(ValueError, match="sigma must be a number"):
                fn(x, wrong)
        with pytest.raises(ValueError, match="mask dtype"):
            fn(x, sigmas, mask=torch.ones(4, 8, 8))
        with pytest.raises(ValueError, match="mask shape"):
            fn(x, sigmas, mask=torch.ones(4, 8, 9, dtype=torch.uint8))
        for fine in (sigmas, sigmas[:1], torch.tensor(1.0), 1.0, 0, 4):      # everything above came first: only now would the GPU be touched
            with pytest.raises(ValueError, match="runs on a CUDA"):
                fn(x, fine)
        with pytest.raises(ValueError, match="runs on a CUDA"):      # a CHW tile: N = 1
            fn(x[0], torch.ones(1))
    with pytest.raises(ValueError, match="runs on a CUDA"):      # (the draw of a module without a device follows the tensor)
        aug(x)
    with pytest.raises(ValueError, match="channel_axis"):
        gaussian_blur(x, 1.0, channel_axis=2)
    with pytest.raises(ValueError, match="a masked Gaussian blur takes planar"):
        gaussian_blur(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 1.0, channel_axis=-1, mask="luminosity")
    with pytest.raises(ValueError, match="luminosity_threshold"):
        gaussian_blur(x, 1.0, luminosity_threshold=0.0)


def test_sample_rows():
    n = 4000
    aug = GaussianBlurAugment((0.5, 3.0), generator=torch.Generator().manual_seed(77))
    rows = aug.sample_rows(n, "cpu")
    assert tuple(rows.shape) == (n,) and rows.dtype == torch.float32 and bool(torch.isfinite(rows).all())
    assert float(rows.min()) >= 0.5 and float(rows.max()) <= 3.0 and float(rows.min()) <= 0.5 + 0.05 * 2.5 and float(rows.max()) >= 3.0 - 0.05 * 2.5      # inside the range, and it is used
    assert abs(float(rows.mean()) - 1.75) <= 4.0 * 2.5 / (12.0 * n) ** 0.5      # centred: 4 standard errors of U[0.5, 3]
    # the restated draw: lo + (hi - lo) * u, u = rand(n) -- a seeded generator reproduces
    again = torch.Generator().manual_seed(77)
    u = torch.rand((n,), generator=again, dtype=torch.float32)
    assert torch.equal(rows, 0.5 + 2.5 * u)
    assert torch.equal(GaussianBlurAugment((0.5, 3.0), generator=torch.Generator().manual_seed(77)).sample_rows(n, "cpu"), rows)
    # lo == hi: exactly that sigma, whatever was drawn
    assert torch.equal(GaussianBlurAugment((1.3, 1.3)).sample_rows(7, "cpu"), torch.full((7,), 1.3, dtype=torch.float32))
    # p < 1: one more draw, rand(n) < p, in that order; a tile that is not chosen gets a NaN sigma
    some = GaussianBlurAugment((0.5, 3.0), p=0.3, generator=torch.Generator().manual_seed(77))
    rows_p = some.sample_rows(n, "cpu")
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.3
    assert tuple(rows_p.shape) == (n,) and torch.equal(torch.isnan(rows_p), ~chosen)
    assert torch.equal(rows_p[chosen], rows[chosen])
    share = float(chosen.float().mean())
    assert abs(share - 0.3) <= 4.0 * (0.3 * 0.7 / n) ** 0.5, share      # 4 standard errors of a binomial share
    assert bool(torch.isnan(GaussianBlurAugment(p=0.0).sample_rows(9, "cpu")).all()) and bool(torch.isfinite(GaussianBlurAugment(p=1.0).sample_rows(9, "cpu")).all())
