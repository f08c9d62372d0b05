"""Separation and augmentation with a given source basis and under tissue masks, without a GPU: the numpy restatement
(tests/_separate_numpy.py) with an all-ones mask and the tile's own oracle estimate IS the oracle, and does not depend on what lies under
the mask; the figure that motivates the masked separation (maxC over all pixels of a sparse tile puts the tissue's 99th percentile well
above target_max_conc); the uint8 cases of the GPU tests keep the near-integer share under the cap of the uint8 rule; the new entry
points are declared, exported and bound; the public arguments are refused before any GPU work."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Macenko, MacenkoAugment, StainEstimate, _native, synth
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn
from tests import _separate_numpy as sn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_macenko_separate_apply": 14, "sx_macenko_separate_apply_masked": 15, "sx_macenko_separate_masked": 16, "sx_macenko_augment_masked": 15}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE
TOL_255 = 2.55e-2      # tests/test_macenko_gpu.py
MAXC_RTOL = 1e-4       # tests/test_macenko_gpu.py
LOOSE_SHARE = 0.12     # tests/test_macenko_mask_gpu.py: the cap of the uint8 rule on levels that lie within TOL_255 of an integer


@pytest.fixture(scope="module")
def ref():
    return so.macenko_fit(synth.reference_tile(64, 64).numpy())


def restatement_cases():
    """The (name, uint8 tiles, mask) cases tests/test_separate_apply_gpu.py restates: real crops 0-4 under the rule, a disc and blocks."""
    x = mn.real_crops(256)[:5]
    yield "rule", x, mn.rule_mask(x.numpy())[0]
    yield "disc", x, mm.disc(5, 256, 256)
    yield "blocks", x, mm.blocks(5, 256, 256, 16)


def test_all_ones_restatement_is_the_oracle(ref):
    sm, tmc = ref
    for tiles in (synth.he_batch(3, 64, 64), mn.real_crops(96)[[0, 2, 4]], synth.he_batch(2, 33, 47)):
        x = synth.as_dtype(tiles, torch.float32).numpy()
        n, _, h, w = x.shape
        want, params = so.macenko_transform(x, sm, tmc, return_params=True)
        od = so.optical_density(so.to_unit_float(x))
        full = [so.macenko_tile_params(od[i]) for i in range(n)]
        he, max_c = np.stack([p["he"] for p in full]), np.stack([p["max_c"] for p in full])
        own, own_levels = sn.separate(x, mm.ones(n, h, w), he)
        for i, p in enumerate(full):
            np.testing.assert_array_equal(own[i].reshape(2, -1), p["conc"])
        # own basis: the two stains together rebuild the input's own optical density as far as the plane holds it; normalised: the transform
        conc, levels = sn.separate(x, mm.ones(n, h, w), he, max_c, (sm, tmc))
        od_new = np.einsum("cs,nshw->nchw", sm.astype(np.float32), conc)
        rebuilt = np.clip(so.IO * np.exp(-od_new), 0, 255)
        assert np.abs(rebuilt - want).max() <= TOL_255
        # ... and so does the product of the two images over 240 (exp(-a - b) = exp(-a) exp(-b))
        product = np.clip(levels[0].astype(np.float64) * levels[1].astype(np.float64) / 240.0, 0, 255)
        assert np.abs(product - want).max() <= TOL_255
        # one source row for the batch == that row repeated
        a = sn.separate(x, mm.ones(n, h, w), he[:1], max_c[:1], (sm, tmc))
        b = sn.separate(x, mm.ones(n, h, w), np.repeat(he[:1], n, axis=0), np.repeat(max_c[:1], n, axis=0), (sm, tmc))
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_restatement_ignores_what_lies_under_the_mask(ref):
    sm, tmc = ref
    tiles = synth.background_stripes(synth.he_batch(3, 64, 64))
    for dtype in (torch.uint8, torch.float32):
        x = synth.as_dtype(tiles, dtype).numpy()
        for mask in (mm.disc(3, 64, 64), mm.blocks(3, 64, 64, 8)):
            rows = mm.estimate(x, mask)
            he, max_c = np.stack([r["he"] for r in rows]), np.stack([r["max_c"] for r in rows])
            y = x.copy()
            out_of_mask = np.broadcast_to(~mask[:, None], x.shape)
            y[out_of_mask] = np.random.default_rng(3).integers(0, 256, int(out_of_mask.sum())).astype(np.uint8) if dtype == torch.uint8 else np.nan
            for reference in (None, (sm, tmc)):
                a, b = sn.separate(x, mask, he, max_c, reference), sn.separate(y, mask, he, max_c, reference)
                np.testing.assert_array_equal(a[0], b[0])
                np.testing.assert_array_equal(a[1], b[1])
                assert not np.isnan(b[0]).any() and not np.isnan(b[1]).any()
                # no stain outside the mask: concentrations +0, both images the 240 level
                outside = np.broadcast_to(~mask[:, None], a[0].shape)
                assert (a[0][outside].view(np.uint32) == 0).all()
                assert (a[1][:, np.broadcast_to(~mask[:, None], x.shape)] == 240.0).all()
        # a NaN source row: the whole tile is background, its neighbours are not touched
        he_nan = he.copy()
        he_nan[1] = np.nan
        c, lv = sn.separate(x, mask, he_nan, max_c, (sm, tmc))
        assert (c[1] == 0).all() and (lv[:, 1] == 240.0).all()
        np.testing.assert_array_equal(c[[0, 2]], a[0][[0, 2]])


def tissue_percentiles(conc: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The oracle-rule 99th percentile of both stains' concentrations over the masked-in pixels of one tile."""
    inside = mask.reshape(-1)
    return np.array([so.nearest_rank(conc[s].reshape(-1)[inside], 99) for s in range(2)], dtype=np.float64)


def test_max_c_over_all_pixels_overshoots_on_a_sparse_tile(ref):
    """Real crop 4 (a third tissue under the luminosity rule at 0.8): normalised concentrations C' = C tmc / maxC of the tissue should have
    their 99th percentile at tmc.  With maxC taken over all pixels it lands at 1.30 tmc (H) and 1.20 tmc (E); over the tissue, at tmc."""
    sm, tmc = ref
    for dtype in (torch.uint8, torch.float32):
        x = synth.as_dtype(mn.real_crops(256)[4:5], dtype).numpy()
        rule = mn.rule_mask(mn.real_crops(256)[4:5].numpy())[0]
        assert 0.25 < rule.mean() < 0.45
        plain = so.macenko_tile_params(so.optical_density(so.to_unit_float(x))[0])
        conc_plain, _ = sn.separate(x, mm.ones(1, 256, 256), plain["he"][None], plain["max_c"][None], (sm, tmc))
        over = tissue_percentiles(conc_plain[0], rule[0]) / tmc
        row = mm.estimate(x, rule)[0]
        conc_masked, _ = sn.separate(x, rule, row["he"][None], row["max_c"][None], (sm, tmc))
        exact = tissue_percentiles(conc_masked[0], rule[0]) / tmc
        print(f"crop 4 {dtype}: tissue share {rule.mean():.3f}; 99th percentile of the tissue's C' / tmc: maxC over all pixels {over}, over the tissue {exact}")
        assert (over >= 1.15).all(), over
        assert (np.abs(exact - 1.0) <= MAXC_RTOL).all(), exact


@pytest.mark.parametrize("normalised", [False, True])
def test_uint8_cases_keep_the_near_integer_share_under_the_cap(ref, normalised):
    """The uint8 rule of the GPU tests compares exactly where the restated level is farther than TOL_255 from an integer, and within one
    level elsewhere; it holds only while the second kind stays a small share (LOOSE_SHARE).  A condition on the INPUT, asserted here
    on the restatement for every uint8 case the GPU tests use."""
    reference = ref if normalised else None
    for what, tiles, mask in restatement_cases():
        x = tiles.numpy()
        rows = mm.estimate(x, mask)
        he, max_c = np.stack([r["he"] for r in rows]), np.stack([r["max_c"] for r in rows])
        _, levels = sn.separate(x, mask, he, max_c, reference)
        where = np.broadcast_to(mask[:, None], x.shape)
        for s, stain in enumerate("HE"):
            share = sn.near_integer_share(levels[s], where, TOL_255)      # (un-clamped, as check_output of tests/test_macenko_mask_gpu.py takes them)
            print(f"{what} normalised={normalised} {stain}: near-integer share of the masked-in levels {share:.3f} (cap {LOOSE_SHARE})")
            assert share <= LOOSE_SHARE, (what, stain, share)


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)


def test_new_calls_reject_bad_arguments_before_any_launch():
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        need = int(lib.sx_macenko_workspace_bytes_for(f32, 4, 64, 64, _native.MACENKO_CLASSIC))

        def sep_apply(images=FAKE, stains=FAKE, conc=FAKE, dtype=f32, n=4, he=FAKE, mc=FAKE, n_sources=4, sm=FAKE, tmc=FAKE, flags=0):
            return lib.sx_macenko_separate_apply(images, stains, conc, dtype, n, 64, 64, he, mc, n_sources, sm, tmc, flags, None)

        def sep_apply_masked(images=FAKE, stains=FAKE, conc=FAKE, dtype=f32, n=4, he=FAKE, mc=FAKE, n_sources=4, sm=FAKE, tmc=FAKE, mask=FAKE, flags=0):
            return lib.sx_macenko_separate_apply_masked(images, stains, conc, dtype, n, 64, 64, he, mc, n_sources, sm, tmc, mask, flags, None)

        def sep_masked(images=FAKE, stains=FAKE, conc=FAKE, dtype=f32, n=4, mask=FAKE, sm=FAKE, tmc=FAKE, flags=0, ws=FAKE, nbytes=need):
            return lib.sx_macenko_separate_masked(images, stains, conc, dtype, n, 64, 64, mask, sm, tmc, None, None, flags, ws, nbytes, None)

        def aug_masked(images=FAKE, out=FAKE, dtype=f32, n=4, mask=FAKE, alpha=FAKE, beta=FAKE, sm=FAKE, tmc=FAKE, flags=0, ws=FAKE, nbytes=need):
            return lib.sx_macenko_augment_masked(images, out, dtype, n, 64, 64, mask, alpha, beta, sm, tmc, flags, ws, nbytes, None)

        for call in (sep_apply_masked, sep_masked, aug_masked):
            assert call(mask=None) == BAD and "mask" in _native.last_error(lib), call.__name__
            for flags in (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_SAMPLED, 1 << 20):
                assert call(flags=flags) == BAD and "flags" in _native.last_error(lib), (call.__name__, flags)
        for call in (sep_apply, sep_apply_masked, sep_masked, aug_masked):
            assert call(flags=_native.MACENKO_CLASSIC, images=None) == BAD      # (CLASSIC is accepted: the next check answers)
            assert call(n=0) == BAD and call(dtype=17) == DTYPE, call.__name__
            assert call(sm=None) == BAD and call(tmc=None) == BAD, call.__name__      # (one of the reference pair)
            assert call(flags=_native.MACENKO_OUT_BF16) == BAD and call(dtype=u8, flags=_native.MACENKO_OUT_BF16 | _native.MACENKO_OUT_F16) == BAD
        assert sep_apply(flags=_native.MACENKO_SAMPLED) == BAD and sep_apply(flags=1 << 20) == BAD
        for call in (sep_apply, sep_apply_masked):
            assert call(stains=None, conc=None) == BAD and "both null" in _native.last_error(lib)
            assert call(he=None) == BAD and call(mc=None) == BAD      # (normalise mode needs source_max_c)
            for n_sources in (0, 2, 3, 5, -1):
                assert call(n_sources=n_sources) == BAD and "n_sources" in _native.last_error(lib), n_sources
        assert sep_masked(stains=None, conc=None) == BAD
        assert sep_masked(nbytes=need - 1) == WORKSPACE and sep_masked(ws=None) == WORKSPACE
        assert aug_masked(out=None) == BAD and aug_masked(alpha=None) == BAD and aug_masked(beta=None) == BAD
        assert aug_masked(nbytes=need - 1) == WORKSPACE and aug_masked(ws=None) == WORKSPACE


def fitted(**kwargs) -> Macenko:
    norm = Macenko(device="cuda", **kwargs)
    norm._stain_matrix, norm._target_max_conc = torch.rand(3, 2), torch.rand(2)
    norm._is_fitted = True
    return norm


BAD_MASKS = [(torch.ones(4, 8, 10, dtype=torch.float32), "dtype"), (torch.ones(4, 8, 10, dtype=torch.int64), "dtype"),
             (torch.ones(4, 10, 8, dtype=torch.uint8), "shape"), (torch.ones(3, 8, 10, dtype=torch.uint8), "shape"),
             (torch.ones(4, 3, 8, 10, dtype=torch.uint8), "shape"), (torch.ones(4, 8, 10, dtype=torch.uint8), "device"),
             (torch.ones(4, 1, 8, 10, dtype=torch.bool), "device"), (np.ones((4, 8, 10), dtype=np.uint8), "tensor"), ("otsu", "mask")]
BAD_SOURCES = [((torch.rand(3, 3, 2), torch.rand(3, 2)), "stain_matrices"), ((torch.rand(4, 2, 3), torch.rand(4, 2)), "stain_matrices"),
               ((torch.rand(4, 3, 2), torch.rand(3, 2)), "max_concentrations"), ((torch.rand(3, 2), torch.rand(1, 3)), "max_concentrations"),
               (torch.rand(4, 3, 2), "source must be"), ((torch.rand(4, 3, 2),), "source must be"), ("slide", "source must be")]


def test_separate_arguments_are_refused_before_any_gpu_work():
    x = torch.zeros(4, 3, 8, 10, dtype=torch.uint8)
    good = (torch.rand(4, 3, 2), torch.rand(4, 2))
    for kwargs in ({}, {"mask": "luminosity"}):
        norm = fitted(**kwargs)
        for mask, what in BAD_MASKS:
            with pytest.raises(ValueError, match=what):
                norm.separate(x, mask=mask)
            with pytest.raises(ValueError, match=what):
                norm.separate(x, source=good, mask=mask)
        for source, what in BAD_SOURCES:
            with pytest.raises(ValueError, match=what):
                norm.separate(x, source=source)
            with pytest.raises(ValueError, match=what):
                norm.separate(x, source=source, mask="luminosity")
        # a source without maxC cannot be normalised to the reference; in its own basis it can (the error below is the next check's)
        with pytest.raises(ValueError, match="max_concentrations"):
            norm.separate(x, source=(good[0], None))
        with pytest.raises(ValueError, match="C=3"):
            norm.separate(torch.zeros(4, 8, 10, 3, dtype=torch.uint8), source=good, mask="luminosity")
        with pytest.raises(ValueError, match="stains, concentrations"):
            norm.separate(x, source=good, stains=False)
    with pytest.raises(ValueError, match="approximate"):
        fitted(precision="sampled").separate(x, mask="luminosity")
    with pytest.raises(ValueError, match="own_basis=False"):
        Macenko(device="cuda").separate(x, source=good, own_basis=False)


def test_augment_arguments_are_refused_before_any_gpu_work():
    for bad in ("otsu", "", 3, torch.ones(1, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask"):
            MacenkoAugment(mask=bad)
    for bad in (0.0, 1.0, float("nan"), "high"):
        with pytest.raises(ValueError, match="luminosity_threshold"):
            MacenkoAugment(mask="luminosity", luminosity_threshold=bad)
    for source, what in BAD_SOURCES:
        if isinstance(source, tuple) and len(source) == 2 and tuple(source[0].shape[-2:]) == (3, 2) and source[1].shape[0] == source[0].shape[0]:
            continue      # (a well-formed pair of three rows: only the batch can refuse it, below)
        with pytest.raises(ValueError, match=what):
            MacenkoAugment(source=source)
    with pytest.raises(ValueError, match="max_concentrations"):
        MacenkoAugment(source=(torch.rand(3, 2), None), normalizer=fitted())      # normalise mode scales with maxC
    x = torch.zeros(4, 3, 8, 10, dtype=torch.uint8)
    est = StainEstimate(torch.rand(1, 3, 2), torch.rand(1, 2), None)
    for module in (MacenkoAugment(device="cuda"), MacenkoAugment(device="cuda", mask="luminosity"), MacenkoAugment(device="cuda", source=est),
                   MacenkoAugment(device="cuda", source=(torch.rand(3, 2), None), mask="luminosity")):
        for mask, what in BAD_MASKS:
            with pytest.raises(ValueError, match=what):
                module(x, mask=mask)
        with pytest.raises(ValueError, match="alpha"):
            module(x, alpha=torch.ones(3, 2), mask="luminosity")
    with pytest.raises(ValueError, match="stain_matrices"):
        MacenkoAugment(device="cuda", source=(torch.rand(3, 3, 2), torch.rand(3, 2)))(x)      # three rows for four tiles
    text = repr(MacenkoAugment(device="cuda", mask="luminosity", luminosity_threshold=0.75, source=est))
    assert "mask='luminosity'" in text and "0.75" in text and "given (1 row)" in text
    assert "mask=None" in repr(MacenkoAugment()) and "per-tile estimate" in repr(MacenkoAugment())
