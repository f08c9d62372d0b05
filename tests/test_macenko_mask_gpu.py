"""Tissue masks for Macenko on the GPU (include/stainx_hip.h: sx_macenko_estimate_masked / _transform_masked / _apply_masked): against the
numpy restatement of the reference's algorithm on the masked-in pixels (tests/_macenko_masked_numpy.py) within the project's own bounds,
the identities bit for bit, degenerate groups, the slow exact select under a mask, the pooled fit, and the plumbing."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Macenko, StainEstimate, _native, synth, tissue_mask
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC
TOL_255 = 2.55e-2      # float32 output on 0-255: the project's parity bound (tests/test_macenko_gpu.py, tests/test_apply_gpu.py)
HALF_BOUND = {torch.bfloat16: 1.0, torch.float16: 0.125}      # 16-bit outputs: tests/test_apply_gpu.py's rule for the same fold
HALF_SHARE = 2e-3
LOOSE_SHARE = 0.12     # uint8: the share of pixels that may fall under the "within one level" half of tests/test_apply_gpu.py's rule
HE_ATOL, MAXC_RTOL = 5e-5, 1e-4      # tests/test_macenko_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev)


@pytest.fixture(scope="module")
def ref():
    he, mc = so.macenko_fit(synth.reference_tile(64, 64).numpy())
    return torch.from_numpy(he), torch.from_numpy(mc)


@pytest.fixture(scope="module")
def real():
    """The six real crops, their rule masks (made on the CPU by the oracle's L), and the restatement's rows under the rule: computed once."""
    x = mn.real_crops(256)
    rule = mn.rule_mask(x.numpy())[0]
    return x, rule


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def unaligned_copy(x: torch.Tensor) -> torch.Tensor:
    """The same values, dense, one element behind an aligned address."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    return view


def mask_t(mask: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(mask.astype(np.uint8)).to(dev)


def inside(mask: np.ndarray, like) -> np.ndarray:
    return np.broadcast_to(mask[:, None], tuple(like.shape))


def check_rows(got: dict, rows: list[dict], what) -> None:
    """HE, maxC, the selection count and the masked-in count of every row against the restatement, where at least 3 masked-in pixels pass the
    filter.  Where those pixels span no plane (a constant tile: zero covariance, so the restated HE and maxC are the eigenvectors of a zero
    matrix, mm.plane_defined) only the two counts are compared; such a tile goes through the identities, as the fallback tiles do."""
    he, mc, kept, n_in = (got[k].cpu().numpy() for k in ("he", "max_c", "tissue", "mask_pixels"))
    for i, row in enumerate(rows):
        assert int(n_in[i]) == row["n_in"], (what, i)
        if row["kept"] < 3:
            continue      # (fallback tiles depend on the eigenvector sign convention: checked through the identities)
        if not row["plane"]:
            print(f"{what} row {i}: masked-in {row['n_in']}, kept {row['n_sel']}, one colour: no plane, counts only")
            assert int(kept[i]) == row["n_sel"], (what, i)
            continue
        e_he, e_mc = np.abs(he[i] - row["he"]).max(), np.abs(mc[i] / row["max_c"] - 1).max()
        print(f"{what} row {i}: masked-in {row['n_in']}, kept {row['n_sel']}, |HE - restated| {e_he:.2e} (bound {HE_ATOL}), maxC rel {e_mc:.2e} (bound {MAXC_RTOL})")
        assert int(kept[i]) == row["n_sel"], (what, i)
        np.testing.assert_allclose(he[i], row["he"], rtol=0, atol=HE_ATOL, err_msg=str((what, i)))
        np.testing.assert_allclose(mc[i], row["max_c"], rtol=MAXC_RTOL, atol=0, err_msg=str((what, i)))


def check_output(got: torch.Tensor, levels: np.ndarray, where: np.ndarray, dt: torch.dtype, what) -> None:
    """The masked-in output against the restated float32 levels, by the rule of the element type (tests/test_apply_gpu.py)."""
    got = got.cpu()
    if dt == torch.float32:
        err = np.abs(got.numpy() - np.clip(levels, 0, 255))[where].max()
        print(f"{what} float32: max |out - restated| on masked-in pixels {err:.3e} (bound {TOL_255})")
        assert err <= TOL_255, what
    elif dt == torch.uint8:
        want = so.restore_dtype(levels, np.uint8, in_0_255=True)
        near = np.abs(levels - np.rint(levels)) <= np.float32(TOL_255)
        assert near[where].mean() <= LOOSE_SHARE, what
        g = got.numpy()
        assert np.array_equal(g[where & ~near], want[where & ~near]), what
        assert np.abs(g.astype(np.int16) - want.astype(np.int16))[where].max() <= 1, what
    else:
        want = torch.from_numpy(np.clip(levels, 0, 255)).to(dt)
        diff = (got.double() - want.double()).abs().numpy()[where]
        print(f"{what} {dt}: max diff {diff.max()}, share differing {(diff > 0).mean():.2e}")
        assert diff.max() <= HALF_BOUND[dt] and (diff > 0).mean() < HALF_SHARE, what


def background_expected(x: torch.Tensor, unit: bool, out_dtype=None) -> torch.Tensor:
    """The background rule on the CPU: the input's level on 0-255 (the byte; x * 255 in float32), clamped, cast, optionally / 255."""
    if x.dtype == torch.uint8:
        level = x.float()
        res = level / 255.0 if unit else level
        return res.to(out_dtype if out_dtype is not None else (torch.float32 if unit else torch.uint8))
    level = (x.float() * 255.0).clamp(0.0, 255.0)
    if x.dtype == torch.float64:
        return level.double() / 255.0 if unit else level.double()
    cast = level.to(x.dtype)
    return (cast.float() / 255.0).to(x.dtype) if unit else cast


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_against_the_restatement(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    sm, tmc = ref
    x8, rule = real
    cases = [("real rule", x8, rule), ("real disc", x8, mm.disc(6, 256, 256)), ("real blocks", x8, mm.blocks(6, 256, 256, 16)),
             ("stripes rule", synth.background_stripes(synth.he_batch(3, 64, 64)), None), ("odd 33x47 blocks", synth.he_batch(2, 33, 47), mm.blocks(2, 33, 47, 5)),
             ("30x30 disc", synth.he_batch(3, 30, 30), mm.disc(3, 30, 30)), ("5x4", synth.he_batch(1, 5, 4), mm.blocks(1, 5, 4, 2, share=0.8)),
             # he_batch below 16 x 16 is one colour (no plane to compare): the same shape and mask once more over a textured tile
             ("5x4 textured", synth.he_batch(1, 40, 32)[:, :, 4::8, 4::8].contiguous(), mm.blocks(1, 5, 4, 2, share=0.8))]
    for what, tiles, mask in cases:
        x = synth.as_dtype(tiles, dt)
        xn = mn.oracle_input(x)
        if mask is None:
            mask = mn.rule_mask(tiles.numpy())[0]
        levels, rows = mm.transform_levels(xn, sm.numpy(), tmc.numpy(), mask, signs="positive_sum")
        m = mask_t(mask, dev)
        got = be.estimate_masked(x.to(dev), m)
        check_rows(got, rows, f"{what} {name}")
        usable = np.array([r["kept"] >= 3 and r["plane"] for r in rows])
        where = inside(mask, x) & usable[:, None, None, None]
        out = be.transform_masked(x.to(dev), sm, tmc, m)
        if usable.any():
            check_output(out, levels, where, dt, f"{what} transform")
        assert same_bits(out.cpu()[~inside(mask, x)], background_expected(x, False)[~inside(mask, x)]), what
        applied = be.apply_masked(x.to(dev), got["he"], got["max_c"], sm, tmc, m)
        assert same_bits(applied, out), what


def test_one_big_tile_and_unaligned_pointers(dev, be, ref):
    sm, tmc = ref
    tile = synth.he_batch(1, 512, 512, seed0=31)
    mask = mm.blocks(1, 512, 512, 32)
    levels, rows = mm.transform_levels(tile.float().numpy() / np.float32(255), sm.numpy(), tmc.numpy(), mask, signs="positive_sum")
    x = synth.as_dtype(tile, torch.float32).to(dev)
    m = mask_t(mask, dev)
    got = be.estimate_masked(x, m)
    check_rows(got, rows, "512x512")
    out = be.transform_masked(x, sm, tmc, m)
    check_output(out, levels, inside(mask, x), torch.float32, "512x512")
    # image and mask each one element off a 16-byte address, independently: the scalar path, the same estimate and output bits
    for xa, ma in ((unaligned_copy(x), m), (x, unaligned_copy(m)), (unaligned_copy(x), unaligned_copy(m))):
        again = be.estimate_masked(xa, ma)
        assert all(same_bits(again[k], got[k]) for k in got)
        assert same_bits(be.transform_masked(xa, sm, tmc, ma), out)
        assert same_bits(be.apply_masked(xa, got["he"], got["max_c"], sm, tmc, ma), out)


# ------------------------------------------------------------------------------------------------ 2. it matters
def test_the_mask_matters_on_an_edge_tile(dev, be, ref, real):
    sm, tmc = ref
    x8, rule = real
    x = synth.as_dtype(x8[4:5], torch.float32).to(dev)
    m = mask_t(rule[4:5], dev)
    masked, plain = be.estimate_masked(x, m), be.estimate(x)
    ratio = float(masked["max_c"][0, 0] / plain["max_c"][0, 0])
    apart = (be.transform_masked(x, sm, tmc, m) - be.transform(x, sm, tmc, _extra_flags=CLASSIC)).abs().cpu().numpy()[inside(rule[4:5], x)].mean()
    print(f"crop 4: tissue share {rule[4].mean():.3f}, maxC[0] masked / unmasked {ratio:.3f}, mean change of the tissue output {apart:.2f} grey levels")
    assert ratio > 1.2 and apart > 5.0


# ------------------------------------------------------------------------------------------------ 3. identities, bit for bit
@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_all_ones_mask_is_the_unmasked_library(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    sm, tmc = ref
    batches = [real[0][:4], synth.he_batch(2, 33, 47)]
    if dt == torch.float32:
        off = synth.as_dtype(real[0][:4], dt)
        batches.append(off * 0.999 + 0.0004)      # off the 8-bit lattice
    for tiles in batches:
        x = (tiles if tiles.dtype == dt else synth.as_dtype(tiles, dt)).to(dev)
        m = torch.ones((x.shape[0],) + tuple(x.shape[2:]), dtype=torch.uint8, device=dev)
        got, want = be.estimate_masked(x, m), be.estimate(x)
        assert same_bits(got["he"], want["he"]) and same_bits(got["max_c"], want["max_c"]) and same_bits(got["tissue"], want["tissue"])
        assert (got["mask_pixels"] == x.shape[2] * x.shape[3]).all()
        he, mc = be.compute_reference_stain_matrix(x)
        phe, pmc = be.compute_reference_stain_matrix_masked(x, m)
        assert same_bits(phe, he) and same_bits(pmc, mc)
        for unit in (False, True):
            assert same_bits(be.transform_masked(x, sm, tmc, m, normalize_to_0_1=unit), be.transform(x, sm, tmc, normalize_to_0_1=unit, _extra_flags=CLASSIC))
            assert same_bits(be.apply_masked(x, want["he"], want["max_c"], sm, tmc, m, normalize_to_0_1=unit), be.apply(x, want["he"], want["max_c"], sm, tmc, normalize_to_0_1=unit))
        if dt == torch.uint8:
            assert same_bits(be.transform_masked(x, sm, tmc, m, out_dtype=torch.bfloat16), be.transform(x, sm, tmc, out_dtype=torch.bfloat16, _extra_flags=CLASSIC))


@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_values_under_the_mask_do_not_matter_and_background_is_copied(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    sm, tmc = ref
    x8 = torch.cat([real[0][[1, 2]], synth.background_stripes(synth.he_batch(2, 256, 256))])
    mask = mm.blocks(4, 256, 256, 16, seed=2)
    x = synth.as_dtype(x8, dt)
    m = mask_t(mask, dev)
    est, out = be.estimate_masked(x.to(dev), m), be.transform_masked(x.to(dev), sm, tmc, m)
    assert same_bits(be.apply_masked(x.to(dev), est["he"], est["max_c"], sm, tmc, m), out)
    where = torch.from_numpy(inside(mask, x).copy())
    fills = [synth.noise_u8(tuple(x.shape), 3) if dt == torch.uint8 else synth.as_dtype(synth.noise_u8(tuple(x.shape), 3), dt)]
    if dt != torch.uint8:
        fills += [torch.full_like(x, float("nan")), torch.full_like(x, float("inf")), torch.full_like(x, float("-inf"))]
    for fill in fills:
        y = torch.where(where, x, fill)
        again = be.estimate_masked(y.to(dev), m)
        assert all(same_bits(again[k], est[k]) for k in est)
        pooled_a, pooled_b = be.estimate_masked(x.to(dev), m, pooled=True), be.estimate_masked(y.to(dev), m, pooled=True)
        assert all(same_bits(pooled_a[k], pooled_b[k]) for k in pooled_a)
        out_y = be.transform_masked(y.to(dev), sm, tmc, m).cpu()
        assert torch.equal(out_y.view(torch.uint8).view(out_y.shape + (-1,))[where], out.cpu().view(torch.uint8).view(out.shape + (-1,))[where])
    # the background: exactly the background rule, / 255 and uint8 -> bf16 included; uint8 -> uint8 is the input's bytes
    options = [dict(), dict(normalize_to_0_1=True)] + ([dict(out_dtype=torch.bfloat16), dict(out_dtype=torch.float16, normalize_to_0_1=True)] if dt == torch.uint8 else [])
    for opt in options:
        want = background_expected(x, opt.get("normalize_to_0_1", False), opt.get("out_dtype"))
        for got in (be.transform_masked(x.to(dev), sm, tmc, m, **opt).cpu(), be.apply_masked(x.to(dev), est["he"], est["max_c"], sm, tmc, m, **opt).cpu()):
            assert got.dtype == want.dtype
            assert torch.equal(got.view(torch.uint8).view(got.shape + (-1,))[~where], want.view(torch.uint8).view(want.shape + (-1,))[~where]), (name, opt)


def test_rule_sources_and_neighbours(dev, be, ref, real):
    sm, tmc = ref
    x = real[0].to(dev)
    made, counts = tissue_mask(x, 0.8)
    # the rule == the explicit mask from tissue_mask()
    by_rule, by_mask = be.estimate_masked(x, None, 0.8), be.estimate_masked(x, made)
    assert all(same_bits(by_rule[k], by_mask[k]) for k in by_rule) and torch.equal(by_rule["mask_pixels"], counts)
    out = be.transform_masked(x, sm, tmc, made)
    assert same_bits(be.transform_masked(x, sm, tmc, None, 0.8), out)
    assert same_bits(be.apply_masked(x, by_mask["he"], by_mask["max_c"], sm, tmc, None, 0.8), out)
    norm = Macenko(device=dev, mask="luminosity")
    norm._stain_matrix, norm._target_max_conc, norm._is_fitted = sm.to(dev), tmc.to(dev), True
    assert same_bits(norm.transform(x), out) and same_bits(Macenko(device=dev).estimate(x, mask=made).stain_matrices, by_mask["he"])
    est = norm.estimate(x)
    assert isinstance(est, StainEstimate) and same_bits(est.tissue_pixels, by_mask["tissue"]) and same_bits(norm.apply(x, est), out)
    assert norm.estimate(x, pooled=True).tissue_pixels is None
    # n_sources = 1 == the row repeated
    one = be.apply_masked(x, by_mask["he"][1:2], by_mask["max_c"][1:2], sm, tmc, made)
    assert same_bits(one, be.apply_masked(x, by_mask["he"][1:2].expand(6, 3, 2), by_mask["max_c"][1:2].expand(6, 2), sm, tmc, made))
    # a tile's masked result does not depend on its batch neighbours
    alone = be.transform_masked(x[4:5], sm, tmc, made[4:5])
    assert same_bits(alone, out[4:5])
    shuffled = be.transform_masked(x[[4, 0, 2]], sm, tmc, made[[4, 0, 2]])
    assert same_bits(shuffled[0:1], alone)


# ------------------------------------------------------------------------------------------------ 4. degenerate groups
def test_degenerate_groups(dev, be, ref, real):
    sm, tmc = ref
    x8 = torch.cat([real[0][[5, 3]], synth.background_stripes(synth.he_batch(3, 256, 256))[1:]])      # glass crop, tissue crop, half glass, all glass
    for dt in (torch.uint8, torch.float32):
        x = synth.as_dtype(x8, dt).to(dev)
        n, _, h, w = x.shape
        for what, mask, has in (("zeros", mm.zeros(n, h, w), False), ("two", mm.exactly(n, h, w, 2), False), ("three", mm.exactly(n, h, w, 3), True)):
            m = mask_t(mask, dev)
            est = be.estimate_masked(x, m)
            assert (est["mask_pixels"].cpu().numpy() == mask.reshape(n, -1).sum(axis=1)).all()
            out = be.transform_masked(x, sm, tmc, m).cpu()
            bg = background_expected(x.cpu(), False)
            if not has:
                assert torch.isnan(est["he"]).all() and torch.isnan(est["max_c"]).all() and (est["tissue"] == 0).all(), what
                assert same_bits(out, bg), what      # every tile copied through
                assert same_bits(be.apply_masked(x, est["he"], est["max_c"], sm, tmc, torch.ones_like(m)).cpu(), bg), what      # a NaN source row: copied, whatever the mask
            else:
                assert torch.isfinite(est["he"]).all() and (est["tissue"] == 3).all(), what
                where = torch.from_numpy(inside(mask, x).copy())
                assert torch.equal(out[~where], bg[~where])
            pooled = be.estimate_masked(x, m, pooled=True)
            if mask.sum() < 3:
                assert torch.isnan(pooled["he"]).all() and torch.isnan(pooled["max_c"]).all() and float(pooled["tissue"][0]) == 0
        # crop 5 and the all-glass tile under the rule: no masked-in pixel -> NaN rows, copied; the others untouched by their neighbours' NaN
        made, counts = tissue_mask(x, 0.8)
        est = be.estimate_masked(x, made)
        empty = (counts < 3).cpu()
        assert bool(empty[0]) and bool(empty[3]) and not bool(empty[1]) and not bool(empty[2])
        assert torch.isnan(est["he"].cpu()[empty]).all() and torch.isfinite(est["he"].cpu()[~empty]).all() and torch.isfinite(est["max_c"].cpu()[~empty]).all()
        out = be.transform_masked(x, sm, tmc, made).cpu()
        assert same_bits(out[empty], background_expected(x.cpu(), False)[empty]) and not torch.isnan(out.float()).any()
        # a mask over glass only: the per-tile fallback takes every masked-in pixel (the sign convention decides HE: checked by the identities)
        glass = torch.zeros_like(made)
        glass[3, :, :128] = 1
        be.estimate_masked(x, glass)
        p = be.tile_params(n)
        assert int(p["use_all"][3]) == 1 and int(p["n_kept"][3]) == 256 * 128
        out_g = be.transform_masked(x, sm, tmc, glass)
        est_g = be.estimate_masked(x, glass)
        assert torch.isfinite(est_g["he"][3]).all() and same_bits(be.apply_masked(x, est_g["he"], est_g["max_c"], sm, tmc, glass), out_g)


# ------------------------------------------------------------------------------------------------ 5. the slow select
def test_slow_exact_select_under_a_mask(dev, ref):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    sm, tmc = ref
    diag = MacenkoHIP(dev, diag=True)      # (the flag below exists in the diagnostic build only)
    tile = synth.he_batch(1, 1024, 512, seed0=55)
    # 8 distinct pixels, 65536 copies each, ~0.7 of them under the mask: every tie group exceeds the 32768 candidates of a slot of this tile
    blocky = tile[:, :, ::256, ::256].repeat_interleave(256, dim=2).repeat_interleave(256, dim=3).contiguous()
    mask = mm.blocks(1, 1024, 512, 48, seed=4, share=0.7)      # (48 does not divide the blocks: the mask cuts through them)
    m = mask_t(mask, dev)
    for x in (blocky, synth.as_dtype(blocky, torch.float32)):
        out = diag.transform_masked(x.to(dev), sm, tmc, m, _extra_flags=_native.MACENKO_NO_TIE_SHORTCUT)
        p = diag.tile_params(1)
        assert int(p["fell_back"][0]) == 0b1111, "expected the whole-tile radix select to run for all four slots"
        fast_out = diag.transform_masked(x.to(dev), sm, tmc, m)
        assert same_bits(fast_out, out)
        levels, rows = mm.transform_levels(mn.oracle_input(x), sm.numpy(), tmc.numpy(), mask, signs="positive_sum")
        np.testing.assert_allclose(p["max_c"][0].numpy(), rows[0]["max_c"], rtol=MAXC_RTOL)
        assert int(p["n_kept"][0]) == rows[0]["n_sel"]
        want = so.restore_dtype(levels, mn.oracle_input(x).dtype, in_0_255=True)
        diff = np.abs(out.cpu().numpy().astype(np.float64) - want.astype(np.float64))[inside(mask, x)].max()
        print(f"blocky {x.dtype}: max |out - restated| {diff:.3e}")
        assert diff <= (1 if x.dtype == torch.uint8 else TOL_255), diff      # (tests/test_macenko_gpu.py's bounds for this tile)


# ------------------------------------------------------------------------------------------------ 6. pooled
def test_pooled_masked_fit(dev, be, real):
    x8, rule = real
    stripes = synth.background_stripes(synth.he_batch(3, 64, 64))
    for what, tiles, mask in (("real rule", x8, rule), ("real blocks", x8, mm.blocks(6, 256, 256, 16)), ("stripes rule", stripes, mn.rule_mask(stripes.numpy())[0])):
        for dt in (torch.uint8, torch.float32, torch.bfloat16):
            x = synth.as_dtype(tiles, dt)
            row = mm.estimate(mn.oracle_input(x), mask, pooled=True, signs="positive_sum")
            got = be.estimate_masked(x.to(dev), mask_t(mask, dev), pooled=True)
            assert got["he"].shape == (1, 3, 2) and got["max_c"].shape == (1, 2)
            check_rows(got, row, f"pooled {what} {dt}")
    ref8 = x8[3:4]
    norm = Macenko(device=dev, mask="luminosity").fit(ref8.to(dev))
    he, mc = mm.fit(ref8.numpy(), rule[3:4], signs="positive_sum")
    np.testing.assert_allclose(norm._stain_matrix.cpu().numpy(), he, rtol=0, atol=HE_ATOL)
    np.testing.assert_allclose(norm._target_max_conc.cpu().numpy(), mc, rtol=MAXC_RTOL, atol=0)
    out = norm.transform(x8.to(dev))
    assert out.dtype == torch.uint8 and torch.equal(out.cpu()[torch.from_numpy(inside(~rule, x8).copy())], x8[torch.from_numpy(inside(~rule, x8).copy())])
    assert same_bits(Macenko(device=dev, mask="luminosity").fit_transform(ref8.to(dev)), norm.transform(ref8.to(dev)))


# ------------------------------------------------------------------------------------------------ 7. plumbing
def test_side_stream_graph_and_shared_workspace(dev, be, ref, real):
    sm, tmc = ref
    x8, rule = real
    x = synth.as_dtype(x8[:4], torch.float32).to(dev)
    m = mask_t(rule[:4], dev)
    m2 = mask_t(mm.blocks(4, 256, 256, 16, seed=8), dev)
    want, want2 = be.transform_masked(x, sm, tmc, m), be.transform_masked(x, sm, tmc, m2)
    est, est2 = be.estimate_masked(x, m), be.estimate_masked(x, m2)
    # masked and unmasked calls alternate on one workspace
    plain = be.transform(x, sm, tmc, _extra_flags=CLASSIC)
    for _ in range(2):
        assert same_bits(be.transform_masked(x, sm, tmc, m), want) and same_bits(be.transform(x, sm, tmc, _extra_flags=CLASSIC), plain)
        again = be.estimate_masked(x, m2)
        assert all(same_bits(again[k], est2[k]) for k in est2) and same_bits(be.estimate(x)["he"], be.estimate(x)["he"])
    # a side stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = be.transform_masked(x, sm, tmc, m)
        applied = be.apply_masked(x, est["he"], est["max_c"], sm, tmc, m)
    side.synchronize()
    assert same_bits(on_side, want) and same_bits(applied, want)
    # captured graphs, replayed after new mask bytes and new source values were written into the same buffers
    smd, tmcd = sm.to(dev), tmc.to(dev)
    mbuf, he_buf, mc_buf = m.clone(), est["he"].clone(), est["max_c"].clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        be.transform_masked(x, smd, tmcd, mbuf)      # (warm-up on the capture stream: its workspace exists before the capture)
        be.apply_masked(x, he_buf, mc_buf, smd, tmcd, mbuf)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap_t = be.transform_masked(x, smd, tmcd, mbuf)
            cap_a = be.apply_masked(x, he_buf, mc_buf, smd, tmcd, mbuf)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(cap_t, want) and same_bits(cap_a, want)
    mbuf.copy_(m2)
    he_buf.copy_(est2["he"])
    mc_buf.copy_(est2["max_c"])
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(cap_t, want2) and same_bits(cap_a, want2)


def test_c_abi_argument_errors_enqueue_nothing(dev, be, ref):
    lib = _native.require()
    sm, tmc = (t.to(dev) for t in ref)
    x = synth.as_dtype(synth.he_batch(2, 64, 64), torch.float32).to(dev)
    m = torch.ones(2, 64, 64, dtype=torch.uint8, device=dev)
    out = torch.full_like(x, -7.0)
    he, mc = torch.full((2, 3, 2), -7.0, device=dev), torch.full((2, 2), -7.0, device=dev)
    code = _native.DTYPE_CODES[torch.float32]
    ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, 2, 64, 64, CLASSIC)), dtype=torch.uint8, device=dev)
    stream = _native.stream_ptr(dev)
    for mask_ptr, flags in ((None, 0), (m.data_ptr(), _native.MACENKO_CHANNELS_LAST), (m.data_ptr(), _native.MACENKO_SAMPLED)):
        assert lib.sx_macenko_transform_masked(x.data_ptr(), out.data_ptr(), code, 2, 64, 64, mask_ptr, sm.data_ptr(), tmc.data_ptr(), flags, ws.data_ptr(), ws.numel(), stream) == _native.SX_ERR_BAD_ARG
        assert _native.last_error(lib)
        assert lib.sx_macenko_estimate_masked(x.data_ptr(), code, 2, 64, 64, mask_ptr, 0, he.data_ptr(), mc.data_ptr(), None, None, flags, ws.data_ptr(), ws.numel(), stream) == _native.SX_ERR_BAD_ARG
        assert lib.sx_macenko_apply_masked(x.data_ptr(), out.data_ptr(), code, 2, 64, 64, he.data_ptr(), mc.data_ptr(), 2, None, None, sm.data_ptr(), tmc.data_ptr(), mask_ptr, flags, stream) == _native.SX_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (he == -7.0).all() and (mc == -7.0).all()
