"""HSV colour augmentation without a GPU: the two entry points are declared and exported, their argument errors at the C ABI return before
anything is enqueued, the float64 restatement of the pixel rule (tests/_hsv_numpy.py) is held to the standard library's ``colorsys``, the
identity row returns every uint8 level exactly under the output rule, and ``HSVAugment`` validates and draws what it says."""
from __future__ import annotations

import colorsys
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import HSVAugment, _native, adjust_hsv
from tests import _hsv_numpy as hn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_hsv_apply": 10, "sx_hsv_apply_masked": 11}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
COLORSYS_TOL = 1e-9      # on [0, 1]: two float64 evaluations of the same rational map


def test_declared_exported_and_public():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.ABI_VERSION == 1
    for name in ("HSVAugment", "adjust_hsv"):
        assert name in stainx_amd.__all__ and hasattr(stainx_amd, name)
    assert isinstance(HSVAugment(), torch.nn.Module) and callable(adjust_hsv)


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, rows=FAKE, n_rows=3, flags=0):
        return lib.sx_hsv_apply(images, out, dtype, n, h, w, rows, n_rows, flags, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, rows=FAKE, n_rows=3, mask=FAKE, flags=0):
        return lib.sx_hsv_apply_masked(images, out, dtype, n, h, w, rows, n_rows, mask, flags, None)

    for fn in (call, masked):
        for name in ("images", "out", "rows"):
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


# ------------------------------------------------------------------ the restatement against colorsys
def _colorsys(levels: np.ndarray, row) -> np.ndarray:
    dh, a_s, b_s, a_v, b_v = (float(np.float32(v)) for v in row)
    out = np.empty_like(levels)
    for i, (r, g, b) in enumerate(levels / 255.0):
        h, s, v = colorsys.rgb_to_hsv(r, g, b)
        out[i] = colorsys.hsv_to_rgb((h + dh) % 1.0, min(max(a_s * s + b_s, 0.0), 1.0), min(max(a_v * v + b_v, 0.0), 1.0))
    return out


def _cpu_pixels() -> np.ndarray:
    """A few thousand seeded pixels (uint8 levels and float32 values), all 256 greys, pixels with two equal channels (the sector
    boundaries: hue 0, 1/6, ... and the ties of the max), black and white -- as float64 levels."""
    rng = np.random.default_rng(41)
    seeded = rng.integers(0, 256, size=(3000, 3)).astype(np.float64)
    floats = rng.random((2000, 3), dtype=np.float32).astype(np.float64) * 255.0
    greys = np.repeat(np.arange(256, dtype=np.float64)[:, None], 3, axis=1)
    pairs = rng.integers(0, 256, size=(600, 2)).astype(np.float64)
    equal = np.concatenate([pairs[:, [0, 0, 1]], pairs[:, [0, 1, 0]], pairs[:, [1, 0, 0]]])
    return np.concatenate([seeded, floats, greys, equal])


ROWS_CPU = hn.ROWS + (hn.IDENTITY, (-0.75, 1.0, 0.0, 1.0, 0.0), (3.25, 0.9, 0.05, 1.05, -0.02), (1.0 / 6.0, 1.0, 0.0, 1.0, 0.0), (-1.0 / 3.0, 2.0, -0.5, 0.5, 0.5))


@pytest.mark.parametrize("row", ROWS_CPU, ids=[f"row{i}" for i in range(len(ROWS_CPU))])
def test_restatement_agrees_with_colorsys(row):
    levels = _cpu_pixels()
    got, copied = hn.levels64(levels, row)
    assert not copied.any() and got.min() >= 0.0 and got.max() <= 255.0
    err = float(np.abs(got / 255.0 - _colorsys(levels, row)).max())
    print(f"restatement against colorsys, row {row}: max |diff| {err:.3e} on [0, 1]")
    assert err <= COLORSYS_TOL, err


def test_identity_row_returns_every_level_exactly_and_copies_are_the_background_rule():
    levels = _cpu_pixels()
    levels = levels[(levels == np.rint(levels)).all(axis=1)]      # the uint8 pixels
    got, _ = hn.levels64(levels, hn.IDENTITY)
    assert np.array_equal(hn.to_output(got, torch.uint8, torch.uint8, False).numpy(), levels.astype(np.uint8))
    assert np.array_equal(hn.float32_emulation(levels, hn.IDENTITY).round().astype(np.uint8), levels.astype(np.uint8))
    assert torch.equal(hn.to_output(got, torch.uint8, torch.float32, True), torch.from_numpy(levels.astype(np.float32)) / 255.0)
    # a NaN member copies the pixel (the NaN itself through the clamp: 0), and so does a non-finite row; an infinity is clamped, not copied
    odd = np.array([[np.nan, 100.0, 50.0], [10.0, np.inf, 20.0], [300.0, -5.0, 128.0]])
    out, copied = hn.levels64(odd, hn.ROWS[0])
    assert copied.tolist() == [True, False, False] and out[0].tolist() == [0.0, 100.0, 50.0]
    assert np.array_equal(out[1:], hn.levels64(np.array([[10.0, 255.0, 20.0], [255.0, 0.0, 128.0]]), hn.ROWS[0])[0])
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(5):
            row = list(hn.ROWS[1])
            row[k] = bad
            out, copied = hn.levels64(odd, row)
            assert copied.all() and out.tolist() == [[0.0, 100.0, 50.0], [10.0, 255.0, 20.0], [255.0, 0.0, 128.0]]


def test_float32_emulation_stays_close_to_float64():
    """The rule in numpy float32 with correctly rounded divisions stays within 2.2e-4 levels of float64 on the four rows (printed): the
    uint8 band's 1e-3 levels of slack is five times that."""
    levels = _cpu_pixels()
    for row in hn.ROWS:
        err = float(np.abs(hn.float32_emulation(levels, row).astype(np.float64) - hn.levels64(levels, row)[0]).max())
        print(f"float32 emulation against float64, row {row}: max |diff| {err:.3e} levels")
        assert err <= 1e-3, err      # (the slack of the uint8 band of the GPU test)


# ------------------------------------------------------------------ the module
def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"hue": 0.51}, "hue"), ({"hue": -0.1}, "hue"), ({"hue": float("nan")}, "hue"), ({"hue": "wide"}, "hue"), ({"saturation": 1.0}, "saturation"),
                         ({"saturation": -0.2}, "saturation"), ({"saturation": float("inf")}, "saturation"), ({"value": 1.0}, "value"), ({"value": -1e-3}, "value"),
                         ({"saturation_shift": -0.1}, "saturation_shift"), ({"saturation_shift": float("inf")}, "saturation_shift"), ({"value_shift": -0.1}, "value_shift"),
                         ({"value_shift": float("nan")}, "value_shift"), ({"p": 1.5}, "p must"), ({"p": -0.1}, "p must"), ({"p": float("nan")}, "p must"),
                         ({"mask": "otsu"}, "mask must be"), ({"luminosity_threshold": 1.5}, "luminosity_threshold"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            HSVAugment(**kwargs)
    aug = HSVAugment(0.5, 0.0, 0.999, saturation_shift=2.0, p=0.0)      # the closed and the open ends
    assert (aug.hue, aug.saturation, aug.value, aug.saturation_shift, aug.value_shift, aug.p) == (0.5, 0.0, 0.999, 2.0, 0.0, 0.0)
    assert "hue=0.5" in repr(aug) and "p=0.0" in repr(aug) and "saturation_shift=2.0" in repr(aug) and "normalize_to_0_1=True" in repr(aug)


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    rows = torch.tensor([hn.IDENTITY] * 4)
    aug = HSVAugment()
    for fn in (lambda *a, **k: adjust_hsv(*a, **k), lambda img, r, **k: aug(img, r, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), rows)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), rows)
        for wrong in (torch.zeros(4, 4), torch.zeros(3, 5), torch.zeros(5, 1), [0.0, 1.0, 0.0, 1.0, 0.0]):
            with pytest.raises(ValueError, match="rows must be"):
                fn(x, wrong)
        with pytest.raises(ValueError, match="mask dtype"):
            fn(x, rows, mask=torch.ones(4, 8, 8))
        with pytest.raises(ValueError, match="mask shape"):
            fn(x, rows, mask=torch.ones(4, 8, 9, dtype=torch.uint8))
        with pytest.raises(ValueError, match="runs on a CUDA"):      # everything above came first: only now would the GPU be touched
            fn(x, rows)
    with pytest.raises(ValueError, match="channel_axis"):
        adjust_hsv(x, rows, channel_axis=2)
    with pytest.raises(ValueError, match="planar"):
        adjust_hsv(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), rows, channel_axis=-1, mask="luminosity")
    with pytest.raises(ValueError, match="luminosity_threshold"):
        adjust_hsv(x, rows, luminosity_threshold=0.0)


def test_sample_rows():
    n = 4000
    aug = HSVAugment(0.05, 0.1, 0.2, saturation_shift=0.03, value_shift=0.04, generator=torch.Generator().manual_seed(77))
    rows = aug.sample_rows(n, "cpu")
    assert tuple(rows.shape) == (n, 5) and rows.dtype == torch.float32 and bool(torch.isfinite(rows).all())
    centre, reach = torch.tensor(hn.IDENTITY), torch.tensor([0.05, 0.1, 0.03, 0.2, 0.04])
    off = (rows - centre).abs()
    assert bool((off <= reach + 2.0**-22).all()) and bool((off.max(dim=0).values >= 0.95 * reach).all())      # inside the ranges, and they are used
    assert bool(((rows - centre).mean(dim=0).abs() <= 4.0 * reach / (3.0 * n) ** 0.5).all())      # centred: 4 standard errors of U[-reach, reach]
    # the restated draw: identity + magnitude * (2 u - 1), u = rand((n, 5)) -- a seeded generator reproduces
    again = torch.Generator().manual_seed(77)
    u = torch.rand((n, 5), generator=again, dtype=torch.float32)
    assert torch.equal(rows, centre + reach * (2.0 * u - 1.0))
    assert torch.equal(HSVAugment(0.05, 0.1, 0.2, saturation_shift=0.03, value_shift=0.04, generator=torch.Generator().manual_seed(77)).sample_rows(n, "cpu"), rows)
    # every magnitude 0: the identity row exactly, whatever was drawn
    assert torch.equal(HSVAugment(0.0, 0.0, 0.0).sample_rows(7, "cpu"), centre.expand(7, 5))
    # p < 1: one more draw, rand(n) < p, in that order; a tile that is not chosen gets a NaN row
    some = HSVAugment(0.05, 0.1, 0.2, saturation_shift=0.03, value_shift=0.04, p=0.3, generator=torch.Generator().manual_seed(77))
    rows_p = some.sample_rows(n, "cpu")
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.3
    assert torch.equal(torch.isnan(rows_p).all(dim=1), ~chosen) and torch.equal(torch.isnan(rows_p).any(dim=1), ~chosen)
    assert torch.equal(rows_p[chosen], rows[chosen])
    share = float(chosen.float().mean())
    assert abs(share - 0.3) <= 4.0 * (0.3 * 0.7 / n) ** 0.5, share      # 4 standard errors of a binomial share
    assert bool(torch.isnan(HSVAugment(p=0.0).sample_rows(9, "cpu")).all()) and bool(torch.isfinite(HSVAugment(p=1.0).sample_rows(9, "cpu")).all())
