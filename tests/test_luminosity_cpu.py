"""Luminosity standardisation without a GPU: the three entry points are declared, exported by both libraries and bound with matching
arity; every argument error at the C ABI returns its code before anything is enqueued and every Python ValueError is raised before the
backend is touched; the rank rule; the float64 restatement against a step-by-step LAB round trip through the oracle's conversions; and
``LuminosityEstimate.lightness``."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from oracle import stain_oracle as so
from stainx_amd import LuminosityEstimate, LuminosityStandardizer, _native
from tests import _luminosity_numpy as ln

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_luminosity_workspace_bytes": 4, "sx_luminosity_percentile": 13, "sx_luminosity_apply": 9}
FAKE, FAKE2, FAKE3, WS = 1 << 40, 1 << 41, 3 << 40, 7 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(r"(?:int|size_t) " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.require_diag().sx_version() == 1
    for name in ("LuminosityStandardizer", "LuminosityEstimate"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.luminosity, name)
    assert issubclass(LuminosityStandardizer, torch.nn.Module) and LuminosityStandardizer.standardize is LuminosityStandardizer.forward
    assert LuminosityEstimate._fields == ("luminance", "pixels")


def test_c_abi_rejects_bad_arguments_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        need = lib.sx_luminosity_workspace_bytes(u8, 4, 64, 64)
        assert need > 0 and need % 256 == 0
        assert lib.sx_luminosity_workspace_bytes(u8, 0, 64, 64) == 0 and lib.sx_luminosity_workspace_bytes(u8, 4, -1, 64) == 0
        assert lib.sx_luminosity_workspace_bytes(u8, 1 << 40, 64, 64) == 0

        def pct(images=FAKE, dtype=u8, n=4, h=64, w=64, mask=None, pooled=0, percentile=95.0, luminance=FAKE2, pixels=None, ws=WS, nbytes=need):
            return lib.sx_luminosity_percentile(images, dtype, n, h, w, mask, pooled, percentile, luminance, pixels, ws, nbytes, None)

        def app(images=FAKE, out=FAKE3, dtype=u8, n=4, h=64, w=64, luminance=FAKE2, n_sources=1):
            return lib.sx_luminosity_apply(images, out, dtype, n, h, w, luminance, n_sources, None)

        def said(word):
            return word in _native.last_error(lib)

        assert pct(images=None) == BAD and said("images")
        assert pct(luminance=None) == BAD and said("luminance_out")
        assert app(images=None) == BAD and said("images")
        assert app(out=None) == BAD and said("out")
        assert app(luminance=None) == BAD and said("luminance")
        for call in (pct, app):
            assert call(n=0) == BAD and call(n=-2) == BAD and call(h=0) == BAD and call(h=-1) == BAD and call(w=0) == BAD and call(w=-7) == BAD
            assert call(n=1 << 40) == BAD and said("overflow")
            assert call(h=1 << 40, w=1 << 40) == BAD and said("overflow")
            assert call(dtype=17) == DTYPE and call(dtype=-1) == DTYPE and said("dtype")
        assert pct(n=1 << 30, h=1 << 15, w=1 << 15, nbytes=1 << 62) == BAD and said("overflow")
        assert app(n=1 << 30, h=1 << 15, w=1 << 15) == BAD and said("overflow")
        for percentile in (0.0, -1.0, 100.0000001, 101.0, float("inf"), float("-inf"), float("nan")):
            assert pct(percentile=percentile) == BAD and said("percentile"), percentile
        assert pct(ws=None) == WORKSPACE and pct(nbytes=need - 1) == WORKSPACE and pct(nbytes=0) == WORKSPACE and said("workspace")
        assert pct(ws=WS + 64) == WORKSPACE and said("aligned")
        for n_sources in (0, 2, 3, 5, -1):
            assert app(n_sources=n_sources) == BAD and said("n_sources"), n_sources
        assert app(out=FAKE) == BAD and said("in place")
    diag = _native.require_diag()
    need = diag.sx_luminosity_workspace_bytes(u8, 4, 64, 64)
    assert diag.sx_luminosity_percentile_plain(None, u8, 4, 64, 64, None, 0, 95.0, FAKE2, None, WS, need, None) == BAD
    assert diag.sx_luminosity_percentile_plain(FAKE, u8, 4, 64, 64, None, 0, 0.0, FAKE2, None, WS, need, None) == BAD


def test_python_validation_before_the_backend_is_touched():
    for bad in (0, 0.0, -5, 100.5, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="percentile"):
            LuminosityStandardizer(percentile=bad)
    for bad in ("slide", "pooled", None, 1):
        with pytest.raises(ValueError, match="statistics"):
            LuminosityStandardizer(statistics=bad)
    with pytest.raises(ValueError, match="CUDA"):
        LuminosityStandardizer(device="cpu")
    std = LuminosityStandardizer()
    assert std.percentile == 95.0 and std.statistics == "tile" and std.device is None
    assert LuminosityStandardizer(100, "batch").percentile == 100.0
    images = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    for value in (torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 3), torch.zeros(8, 8), np.zeros((2, 3, 8, 8)), None):
        for call in (std.estimate, std.forward, std.standardize, lambda x: std.apply(x, torch.zeros(1))):
            with pytest.raises(ValueError, match="expects"):
                call(value)
    # the string mask raises: the luminosity rule is not a mask mode here
    for call in (lambda m: std.estimate(images, mask=m), lambda m: std(images, mask=m), lambda m: std.standardize(images, m)):
        with pytest.raises(ValueError, match="not a mask mode"):
            call("luminosity")
        for bad_mask in (torch.zeros(2, 8, 8), torch.zeros(2, 8, 9, dtype=torch.uint8), torch.zeros(3, 8, 8, dtype=torch.bool), 1):
            with pytest.raises(ValueError, match="mask"):
                call(bad_mask)
    for bad in (torch.zeros(3), torch.zeros(2, 2), torch.zeros(0), None, 0.5, LuminosityEstimate(torch.zeros(3), torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(ValueError, match="estimate"):
            std.apply(images, bad)
    # there is no CPU path: a CPU tensor without a device is refused, not computed
    for call in (std.estimate, std.forward, lambda x: std.apply(x, torch.zeros(1))):
        with pytest.raises(ValueError, match="CUDA"):
            call(images)
    assert std._engines == {}      # (nothing above reached the backend)


@pytest.mark.parametrize("count", [1, 2, 3, 21, 10 ** 5])
def test_rank_rule(count):
    """k = 1 + rint(0.01 p (|S| - 1)), half to even, against exact rational arithmetic where the product is representable."""
    from fractions import Fraction

    for percentile in (0.5, 50.0, 95.0, 100.0):
        k = ln.rank(count, percentile)
        assert 1 <= k <= count
        product = (0.01 * percentile) * float(count - 1)      # the double the rule rounds
        lower = int(np.floor(product))
        frac = Fraction(product) - lower
        want = lower + (1 if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and lower % 2 == 1) else 0)
        assert k == 1 + want, (count, percentile, k)
    assert ln.rank(count, 100.0) == count      # the maximum
    assert ln.rank(count, 0.5) == 1 + int(np.rint(0.005 * (count - 1)))
    assert ln.rank(0, 95.0) == 0
    # known values: ties go to even
    assert ln.rank(2, 50.0) == 1 and ln.rank(3, 50.0) == 2 and ln.rank(21, 50.0) == 11 and ln.rank(21, 95.0) == 20 and ln.rank(10 ** 5, 95.0) == 95000
    assert ln.rank(4, 50.0) == 3 and ln.rank(6, 50.0) == 3      # 1.5 -> 2, 2.5 -> 2


def test_restatement_is_the_lab_round_trip_with_only_lightness_changed():
    """The restatement against the oracle's float32 conversions step by step -- RGB -> LAB, L*' = min(100 L* / L_p, 100), LAB -> RGB -- on
    crops of the real images.  1e-4 on unit values: the project's bound for a float32 evaluation of this conversion chain."""
    images = ln.real_images()
    for index, (y0, x0) in enumerate(((300, 400), (0, 0), (600, 128), (512, 512), (100, 800), (900, 50))):
        crop = images[index:index + 1, :, y0:y0 + 96, x0:x0 + 80]
        y = np.sort(ln.luminance(crop).reshape(-1))
        for percentile in (50.0, 95.0, 100.0):
            y_p = y[ln.rank(y.size, percentile) - 1]
            mine = ln.standardize_unit(crop, np.array([y_p]))
            theirs = ln.lab_round_trip(crop, y_p, so.rgb_to_lab, so.lab_to_rgb)
            assert np.abs(mine - theirs).max() <= 1e-4, (index, percentile, np.abs(mine - theirs).max())
            # a* and b* are kept where L* was not clipped and the result is inside the gamut
            lab_in, lab_out = so.rgb_to_lab(ln.unit(crop).astype(np.float32)), so.rgb_to_lab(mine.astype(np.float32))
            inside = (mine.min(axis=1) > 0.0) & (mine.max(axis=1) < 1.0)
            assert inside.any()
            assert np.abs(lab_out[:, 1:] - lab_in[:, 1:]).transpose(0, 2, 3, 1)[inside].max() < 2e-2      # (LAB units of 0..255, float32 round trip)
            want_l = np.minimum(lab_in[:, 0] * 100.0 / ln.lightness(y_p), 255.0)
            assert np.abs(lab_out[:, 0] - want_l)[inside].max() < 2e-2


def test_through_copy_rows_and_per_tile_rows():
    images = ln.real_images()[:3, :, 200:232, 200:240]
    rows = np.array([np.nan, 0.0, 0.5])
    out = ln.standardize_unit(images, rows)
    assert np.array_equal(out[0], ln.unit(images)[0]) and np.array_equal(out[1], ln.unit(images)[1])
    assert np.array_equal(out[2:], ln.standardize_unit(images[2:], np.array([0.5])))
    g, through = ln.gain(rows)
    assert through.tolist() == [True, True, False] and g[0] == 1.0 and abs(g[2] - 100.0 / ln.lightness(0.5)) < 1e-15


def test_lightness_of_known_luminances():
    y = torch.tensor([0.0, 0.008856, 0.001, 0.18418651, 0.5, 1.0, float("nan")], dtype=torch.float32)
    est = LuminosityEstimate(y, torch.zeros(7, dtype=torch.int64))
    got = est.lightness
    assert got.dtype == torch.float64 and got.shape == (7,)
    y64 = y.double().numpy()
    want = np.where(y64 > 0.008856, 116.0 * np.cbrt(y64) - 16.0, 116.0 * (7.787 * y64 + 16.0 / 116.0) - 16.0)
    assert np.allclose(got[:6].numpy(), want[:6], rtol=0, atol=1e-12) and torch.isnan(got[6])
    assert abs(got[0].item()) < 1e-12 and got[5].item() == 100.0 and abs(got[3].item() - 50.0) < 1e-4 and abs(got[4].item() - 76.0693) < 1e-3
    assert np.allclose(ln.lightness(y64[:6]), want[:6], rtol=0, atol=1e-12)
