"""Tissue masks for Macenko without a GPU: the numpy restatement with an all-ones mask IS the oracle and does not depend on the values
under the mask; the normaliser's mask arguments are refused before any GPU work; the new entry points are declared, exported by both
libraries and bound with matching arity, and refuse bad arguments before anything is enqueued."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Macenko, _native, synth
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_macenko_estimate_masked": 15, "sx_macenko_transform_masked": 13, "sx_macenko_apply_masked": 16}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE


def inputs():
    yield "stripes", synth.background_stripes(synth.he_batch(3, 64, 64))
    yield "real_96", mn.real_crops(96)[[0, 2, 4]]
    yield "odd", synth.he_batch(2, 33, 47)


def test_all_ones_restatement_is_the_oracle():
    ref_he, ref_mc = so.macenko_fit(synth.reference_tile(64, 64).numpy())
    for what, tiles in inputs():
        for dtype in (torch.uint8, torch.float32):
            x = synth.as_dtype(tiles, dtype).numpy()
            all_in = mm.ones(x.shape[0], x.shape[2], x.shape[3])
            np.testing.assert_array_equal(mm.transform(x, ref_he, ref_mc, all_in), so.macenko_transform(x, ref_he, ref_mc), err_msg=what)
            _, params = so.macenko_transform(x, ref_he, ref_mc, return_params=True)
            for row, p in zip(mm.estimate(x, all_in), params):
                np.testing.assert_array_equal(row["he"], p["he"])
                np.testing.assert_array_equal(row["max_c"], p["max_c"])
                assert row["n_sel"] == p["n_kept"] and row["n_in"] == x.shape[2] * x.shape[3]
            for got, want in zip(mm.fit(x, all_in), so.macenko_fit(x)):
                np.testing.assert_array_equal(got, want, err_msg=what)


def test_restatement_ignores_what_lies_under_the_mask():
    ref_he, ref_mc = so.macenko_fit(synth.reference_tile(64, 64).numpy())
    tiles = synth.background_stripes(synth.he_batch(3, 64, 64))
    for dtype in (torch.uint8, torch.float32):
        x = synth.as_dtype(tiles, dtype).numpy()
        for mask in (mm.disc(3, 64, 64), mm.blocks(3, 64, 64, 8)):
            y = x.copy()
            out_of_mask = np.broadcast_to(~mask[:, None], x.shape)
            y[out_of_mask] = np.random.default_rng(3).integers(0, 256, int(out_of_mask.sum())).astype(np.uint8) if dtype == torch.uint8 else np.nan
            a, b = mm.transform(x, ref_he, ref_mc, mask), mm.transform(y, ref_he, ref_mc, mask)
            inside = np.broadcast_to(mask[:, None], x.shape)
            np.testing.assert_array_equal(a[inside], b[inside])
            for ra, rb in zip(mm.estimate(x, mask) + mm.estimate(x, mask, pooled=True), mm.estimate(y, mask) + mm.estimate(y, mask, pooled=True)):
                np.testing.assert_array_equal(ra["he"], rb["he"])
                np.testing.assert_array_equal(ra["max_c"], rb["max_c"])
                assert (ra["n_sel"], ra["n_in"]) == (rb["n_sel"], rb["n_in"])
            # the background is the input's level through the clamp and cast: the input itself for uint8, x * 255 for floats
            if dtype == torch.uint8:
                np.testing.assert_array_equal(a[out_of_mask], x[out_of_mask])
            else:
                np.testing.assert_array_equal(a[out_of_mask], np.clip(x[out_of_mask] * np.float32(255), 0, 255))


def test_restatement_degenerate_groups():
    x = synth.background_stripes(synth.he_batch(3, 64, 64)).numpy()
    for k, has in ((0, False), (2, False), (3, True)):
        mask = mm.exactly(3, 64, 64, k) if k else mm.zeros(3, 64, 64)
        rows = mm.estimate(x, mask)
        assert all(r["n_in"] == k for r in rows)
        assert all(np.isfinite(r["he"]).all() == has and (r["n_sel"] > 0) == has for r in rows), k
    glass_only = np.zeros((3, 64, 64), dtype=bool)
    glass_only[2] = True      # (the third striped tile is all glass: no pixel passes the OD filter)
    pooled = mm.estimate(x, glass_only, pooled=True)[0]
    assert np.isnan(pooled["he"]).all() and pooled["n_sel"] == 0 and pooled["n_in"] == 64 * 64
    per_tile = mm.estimate(x, glass_only)[2]
    assert per_tile["fallback"] and per_tile["n_sel"] == 64 * 64 and np.isfinite(per_tile["max_c"]).all()


def test_restatement_says_where_there_is_no_plane():
    """One colour under the mask: zero covariance, nothing to compare HE and maxC with; a single level of change in one pixel of a
    channel is rank 1 still; textured tiles and the real crops span a plane by three orders over the floor."""
    flat = synth.he_batch(1, 5, 4).numpy()
    assert len(np.unique(flat.reshape(3, -1), axis=1).T) == 1
    row = mm.estimate(flat, mm.ones(1, 5, 4))[0]
    assert row["kept"] == 20 and not row["plane"]
    flat[0, 1, 2, 2] += 1
    assert not mm.estimate(flat, mm.ones(1, 5, 4))[0]["plane"]
    textured = synth.he_batch(1, 40, 32)[:, :, 4::8, 4::8].contiguous().numpy()
    assert mm.estimate(textured, mm.blocks(1, 5, 4, 2, share=0.8))[0]["plane"]
    for what, tiles in inputs():
        x = tiles.numpy()
        for row in mm.estimate(x, mn.rule_mask(x)[0]) + mm.estimate(x, mn.rule_mask(x)[0], pooled=True):
            assert row["plane"] == (row["kept"] >= 3), what


def fitted(**kwargs) -> Macenko:
    norm = Macenko(device="cuda", **kwargs)
    norm._stain_matrix, norm._target_max_conc = torch.rand(3, 2), torch.rand(2)
    norm._is_fitted = True
    return norm


def test_mask_arguments_are_refused_before_any_gpu_work():
    plain = Macenko(device="cuda")
    assert plain.mask is None and plain.luminosity_threshold == 0.8      # the default is the unmasked library
    masked = Macenko(device="cuda", mask="luminosity", luminosity_threshold=0.75)
    assert masked.mask == "luminosity" and masked.luminosity_threshold == 0.75
    for bad in ("otsu", "", 3, torch.ones(1, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask"):
            Macenko(device="cuda", mask=bad)
    for bad in (0.0, 1.0, -0.2, 1.5, float("nan"), "high", None):
        with pytest.raises(ValueError, match="luminosity_threshold"):
            Macenko(device="cuda", mask="luminosity", luminosity_threshold=bad)
    with pytest.raises(ValueError, match="sampled"):
        Macenko(device="cuda", precision="sampled", mask="luminosity")

    x = torch.zeros(4, 3, 8, 10, dtype=torch.uint8)
    source = (torch.rand(4, 3, 2), torch.rand(4, 2))
    bad_masks = [(torch.ones(4, 8, 10, dtype=torch.float32), "dtype"), (torch.ones(4, 8, 10, dtype=torch.int64), "dtype"),
                 (torch.ones(4, 10, 8, dtype=torch.uint8), "shape"), (torch.ones(3, 8, 10, dtype=torch.uint8), "shape"),
                 (torch.ones(4, 3, 8, 10, dtype=torch.uint8), "shape"), (torch.ones(4, 8, 10, dtype=torch.uint8), "device"),
                 (torch.ones(4, 1, 8, 10, dtype=torch.bool), "device"), (np.ones((4, 8, 10), dtype=np.uint8), "tensor"), ("otsu", "mask")]
    for kwargs in ({}, {"mask": "luminosity"}):
        norm = fitted(**kwargs)
        calls = [norm.fit, norm.transform, norm.fit_transform, lambda images, mask: norm.estimate(images, mask=mask),
                 lambda images, mask: norm.estimate(images, pooled=True, mask=mask), lambda images, mask: norm.apply(images, source, mask=mask)]
        for call in calls:
            for mask, what in bad_masks:
                with pytest.raises(ValueError, match=what):
                    call(x, mask=mask)
    # "sampled" and a mask for one call; the images are checked first where the mask's shape depends on them
    sampled = fitted(precision="sampled")
    for call in (sampled.fit, sampled.transform, lambda images, mask: sampled.apply(images, source, mask=mask)):
        with pytest.raises(ValueError, match="sampled"):
            call(x, mask="luminosity")
    with pytest.raises(ValueError, match="C=3"):
        fitted(mask="luminosity").transform(torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
        Macenko(device="cuda", mask="luminosity").transform(x, mask="luminosity")


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)


def test_masked_calls_reject_bad_arguments_before_any_launch():
    u8, f32 = _native.DTYPE_CODES[torch.uint8], _native.DTYPE_CODES[torch.float32]
    for lib in (_native.require(), _native.require_diag()):
        need = int(lib.sx_macenko_workspace_bytes_for(f32, 4, 64, 64, _native.MACENKO_CLASSIC))

        def estimate(images=FAKE, dtype=f32, n=4, mask=FAKE, pooled=0, he=FAKE, mc=FAKE, flags=0, ws=FAKE, nbytes=need):
            return lib.sx_macenko_estimate_masked(images, dtype, n, 64, 64, mask, pooled, he, mc, None, None, flags, ws, nbytes, None)

        def transform(images=FAKE, out=FAKE, dtype=f32, n=4, mask=FAKE, sm=FAKE, tmc=FAKE, flags=0, ws=FAKE, nbytes=need):
            return lib.sx_macenko_transform_masked(images, out, dtype, n, 64, 64, mask, sm, tmc, flags, ws, nbytes, None)

        def apply(images=FAKE, out=FAKE, dtype=f32, n=4, he=FAKE, mc=FAKE, n_sources=4, alpha=None, beta=None, sm=FAKE, tmc=FAKE, mask=FAKE, flags=0):
            return lib.sx_macenko_apply_masked(images, out, dtype, n, 64, 64, he, mc, n_sources, alpha, beta, sm, tmc, mask, flags, None)

        for call in (estimate, transform, apply):
            assert call(mask=None) == BAD and "mask" in _native.last_error(lib), call.__name__
            for flags in (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_SAMPLED, 1 << 20):
                assert call(flags=flags) == BAD and "flags" in _native.last_error(lib), (call.__name__, flags)
            assert call(flags=_native.MACENKO_CLASSIC, images=None) == BAD      # (CLASSIC is accepted: the next check answers)
            assert call(n=0) == BAD and call(dtype=17) == DTYPE
        for pooled in (0, 1):
            assert estimate(he=None, pooled=pooled) == BAD and estimate(mc=None, pooled=pooled) == BAD
            assert estimate(nbytes=need - 1, pooled=pooled) == WORKSPACE and estimate(ws=None, pooled=pooled) == WORKSPACE and estimate(ws=FAKE + 8, pooled=pooled) == WORKSPACE
        assert estimate(flags=_native.MACENKO_NORMALIZE_0_1) == BAD      # (no output: CLASSIC is the estimate's only flag)
        assert transform(out=None) == BAD and transform(sm=None) == BAD and transform(tmc=None) == BAD
        assert transform(nbytes=need - 1) == WORKSPACE and transform(ws=None) == WORKSPACE
        assert transform(flags=_native.MACENKO_OUT_BF16) == BAD and transform(dtype=u8, flags=_native.MACENKO_OUT_BF16 | _native.MACENKO_OUT_F16) == BAD
        assert transform(dtype=u8, flags=_native.MACENKO_OUT_BF16 | _native.MACENKO_NORMALIZE_0_1, out=None) == BAD
        assert apply(out=None) == BAD and apply(he=None) == BAD and apply(mc=None) == BAD and apply(sm=None) == BAD and apply(alpha=FAKE) == BAD
        assert apply(sm=None, tmc=None) == BAD      # (own basis without factors)
        for n_sources in (0, 2, 3, 5, -1):
            assert apply(n_sources=n_sources) == BAD and "n_sources" in _native.last_error(lib), n_sources
    assert _native.require().sx_macenko_transform_masked(FAKE, FAKE, f32, 4, 64, 64, FAKE, FAKE, FAKE, _native.MACENKO_NO_TIE_SHORTCUT, FAKE, 1 << 40, None) == BAD      # (a diagnostic bit: the product refuses it)
