"""Separation with a given source basis and under tissue masks on the GPU (include/stainx_hip.h: sx_macenko_separate_apply,
sx_macenko_separate_apply_masked, sx_macenko_separate_masked).

* the identities, bit for bit: separate_apply(x, estimate(x)) = separate(x); one source row = that row repeated; an all-ones mask = the
  unmasked call; separate_masked = estimate_masked + separate_apply_masked; the masked H / E images on masked-in pixels = augment_masked
  with alpha = e_i; exact values on masked-out pixels; values under the mask do not matter;
* against the numpy restatement (tests/_separate_numpy.py) from the call's own rows, the rows against tests/_macenko_masked_numpy.py;
* the mask matters on a sparse tile; degenerate groups; workspace, graph capture, side stream; the C ABI; the public method.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Macenko, StainEstimate, _native, synth, tissue_mask
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn
from tests import _separate_numpy as sn
from tests.conftest import TORCH_DTYPES
from tests.test_macenko_mask_gpu import background_expected, check_output, check_rows, inside, mask_t, same_bits, unaligned_copy
from tests.test_separate_gpu import TOL_CONC

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC
ELEM_BYTES = {torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4, torch.float64: 8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev)


@pytest.fixture(scope="module")
def ref(dev):
    he, mc = so.macenko_fit(synth.reference_tile(64, 64).numpy())
    return torch.from_numpy(he).to(dev), torch.from_numpy(mc).to(dev)


@pytest.fixture(scope="module")
def real():
    x = mn.real_crops(256)
    return x, mn.rule_mask(x.numpy())[0]


def work_item_pixels(in_dtype: torch.dtype, out_dtype: torch.dtype, vector: bool = True) -> int:
    """Pixels of one work item of separate_apply_kernel (csrc/macenko.hip: separate_apply_chunk): 256 threads, one pack set of 16 bytes
    of output per lane and plane -- never wider than the input's 16-byte pack -- on the vector paths, sixteen single pixels on the scalar path."""
    if not vector:
        return 256 * 16
    return 256 * min(16 // ELEM_BYTES[out_dtype], 16 // ELEM_BYTES[in_dtype])


def textured_5x4() -> torch.Tensor:
    return synth.he_batch(1, 40, 32)[:, :, 4::8, 4::8].contiguous()


def shapes(real_tiles: torch.Tensor):
    yield "64x64", synth.he_batch(3, 64, 64)
    yield "33x47", synth.he_batch(2, 33, 47)
    yield "30x30", synth.he_batch(3, 30, 30)
    yield "5x4", textured_5x4()
    yield "96x96", synth.he_batch(2, 96, 96, seed0=77)      # (9216 pixels: more than the largest work item, 4096 -- two full items and a partial one)
    yield "real", real_tiles


def masks_for(tiles: torch.Tensor):
    n, _, h, w = tiles.shape
    yield "disc", mm.disc(n, h, w)
    yield "blocks16", mm.blocks(n, h, w, 16)
    yield "blocks5", mm.blocks(n, h, w, 5)
    yield "rule", mn.rule_mask(tiles.numpy())[0]


def finite_scale(max_c: torch.Tensor) -> torch.Tensor:
    """(N, 2) bool: the stain's scale tmc / maxC is finite and non-zero."""
    return torch.isfinite(max_c) & (max_c != 0)


def no_stain_level(in_dtype: torch.dtype, unit: bool, out_dtype=None) -> torch.Tensor:
    """The level of zero concentration, 240, through the output path of a tissue pixel (background_expected's steps after its level)."""
    level = torch.tensor(240.0)
    if in_dtype == torch.uint8:
        res = level / 255.0 if unit else level
        return res.to(out_dtype if out_dtype is not None else (torch.float32 if unit else torch.uint8))
    if in_dtype == torch.float64:
        return level.double() / 255.0 if unit else level.double()
    cast = level.to(in_dtype)
    return (cast.float() / 255.0).to(in_dtype) if unit else cast


def bits(t: torch.Tensor) -> torch.Tensor:
    """Elementwise byte view: (..., element bytes) uint8, to index with a mask over elements."""
    t = t.contiguous()
    return t.view(torch.uint8).view(t.shape + (-1,))


def assert_same_separation(a: dict, b: dict, what, tiles: torch.Tensor | None = None) -> None:
    """Stain images and concentrations bit for bit (of the tiles selected by the (N,) bool `tiles`)."""
    for key in ("stains", "concentrations"):
        if a[key] is None:
            assert b[key] is None, (what, key)
            continue
        x, y = a[key], b[key]
        if tiles is not None:
            x, y = (x[:, tiles], y[:, tiles]) if key == "stains" else (x[tiles], y[tiles])
        assert same_bits(x, y), (what, key)


def options_for(dt: torch.dtype):
    yield {}
    yield {"normalize_to_0_1": True}
    if dt == torch.uint8:
        yield {"out_dtype": torch.bfloat16}
        yield {"out_dtype": torch.float16, "normalize_to_0_1": True}


# ------------------------------------------------------------------------------------------------ 1. the identities, bit for bit
@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_given_the_tiles_own_estimate_is_separate(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    for what, tiles in shapes(real[0]):
        x = synth.as_dtype(tiles, dt).to(dev)
        n = x.shape[0]
        if what == "96x96":
            out_dt = dt
            assert x.shape[2] * x.shape[3] > work_item_pixels(dt, out_dt) and x.shape[2] * x.shape[3] > work_item_pixels(dt, out_dt, vector=False)
        for layout in (False, True):
            xl = x.permute(0, 2, 3, 1).contiguous() if layout else x
            est = be.estimate(xl, channels_last=layout)
            for reference in ((), ref):
                ok = finite_scale(est["max_c"]).all(dim=1) if reference else torch.ones(n, dtype=torch.bool, device=dev)
                assert what == "real" or bool(ok.all()), what
                for opt in options_for(dt):
                    want = be.separate(xl, *reference, concentrations=True, max_conc=True, channels_last=layout, **opt)
                    assert same_bits(want["he"], est["he"]) and same_bits(want["max_c"], est["max_c"]), (what, layout)
                    got = be.separate_apply(xl, est["he"], est["max_c"], *reference, concentrations=True, channels_last=layout, **opt)
                    assert got["stains"].dtype == want["stains"].dtype
                    assert_same_separation(got, want, (what, layout, len(reference), opt), ok)
                    assert same_bits(got["he"], est["he"]) and same_bits(got["max_c"], est["max_c"])
                # images only, concentrations only (their own instantiation: the float pack)
                only = be.separate_apply(xl, est["he"], est["max_c"], *reference, stains=False, concentrations=True, channels_last=layout)
                plain = be.separate(xl, *reference, stains=False, concentrations=True, channels_last=layout)
                assert_same_separation(only, plain, (what, "concentrations only"), ok)
                # own basis needs no maxC
                if not reference:
                    assert_same_separation(be.separate_apply(xl, est["he"], None, channels_last=layout), be.separate(xl, channels_last=layout), (what, "no maxC"))
                # one source row: the result does not depend on n_sources
                one = be.separate_apply(xl, est["he"][:1], est["max_c"][:1], *reference, concentrations=True, channels_last=layout)
                rep = be.separate_apply(xl, est["he"][:1].expand(n, 3, 2).contiguous(), est["max_c"][:1].expand(n, 2).contiguous(), *reference, concentrations=True,
                                        channels_last=layout)
                assert_same_separation(one, rep, (what, "one row"))
                assert one["he"].shape == (n, 3, 2) and one["max_c"].shape == (n, 2) and same_bits(one["he"][n - 1], est["he"][0])
            # images one element off a 16-byte address: the scalar path, the same bits
            if not layout:
                moved = be.separate_apply(unaligned_copy(x), est["he"], est["max_c"], *ref, concentrations=True)
                assert_same_separation(moved, be.separate_apply(x, est["he"], est["max_c"], *ref, concentrations=True), (what, "unaligned images"))


@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_all_ones_mask_is_the_unmasked_call(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    for what, tiles in shapes(real[0]):
        x = synth.as_dtype(tiles, dt).to(dev)
        n, _, h, w = x.shape
        m = torch.ones((n, h, w), dtype=torch.uint8, device=dev)
        est = be.estimate(x)
        for reference in ((), ref):
            pair = reference if reference else (None, None)
            for opt in options_for(dt):
                plain = be.separate(x, *reference, concentrations=True, max_conc=True, **opt)
                masked = be.separate_masked(x, *pair, m, concentrations=True, max_conc=True, **opt)
                assert_same_separation(masked, plain, (what, len(reference), opt))
                assert same_bits(masked["he"], plain["he"]) and same_bits(masked["max_c"], plain["max_c"])
                given = be.separate_apply(x, est["he"], est["max_c"], *reference, concentrations=True, **opt)
                assert_same_separation(be.separate_apply_masked(x, est["he"], est["max_c"], *pair, m, concentrations=True, **opt), given, (what, "apply", opt))
            assert be.separate_masked(x, *pair, m)["max_c"] is None or reference      # (own basis without max_conc: the estimate stops after the stain stage)


# ------------------------------------------------------------------------------------------------ 2. masked identities and exact values
@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_masked_identities_and_background_values(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    for what, tiles in shapes(real[0]):
        x = synth.as_dtype(tiles, dt).to(dev)
        n = x.shape[0]
        zeros = torch.zeros(n, 2, device=dev)
        units = [torch.tensor([[1.0, 0.0]], device=dev).expand(n, 2).contiguous(), torch.tensor([[0.0, 1.0]], device=dev).expand(n, 2).contiguous()]
        for mask_name, mask in masks_for(tiles):
            m = mask_t(mask, dev)
            est = be.estimate_masked(x, m)
            where = torch.from_numpy(inside(mask, x).copy()).to(dev)
            for reference in ((None, None), ref):
                normalised = reference[0] is not None
                for opt in options_for(dt):
                    tag = (what, mask_name, normalised, opt)
                    got = be.separate_masked(x, *reference, m, concentrations=True, max_conc=True, **opt)
                    # separate_masked = estimate_masked + separate_apply_masked
                    assert same_bits(got["he"], est["he"]) and same_bits(got["max_c"], est["max_c"]), tag
                    assert_same_separation(be.separate_apply_masked(x, est["he"], est["max_c"], *reference, m, concentrations=True, **opt), got, tag)
                    # masked-out pixels hold no stain: concentrations +0.0f as bits, images the 240 level
                    outside_c = ~where[:, :2]
                    assert int(got["concentrations"].view(torch.int32)[outside_c].abs().max().item() if bool(outside_c.any()) else 0) == 0, tag
                    level = no_stain_level(dt, opt.get("normalize_to_0_1", False), opt.get("out_dtype")).to(dev)
                    assert got["stains"].dtype == level.dtype, tag
                    for s in range(2):
                        assert (bits(got["stains"][s])[~where] == bits(level.reshape(1))[0]).all(), (tag, s)
                    # the masked H / E image on masked-in pixels = augment_masked with alpha = e_i, beta = 0, where the other stain's scale is finite
                    has = torch.isfinite(est["he"]).all(dim=2).all(dim=1)
                    fine = has & (finite_scale(est["max_c"]).all(dim=1) if normalised else True)
                    pick = where & fine.view(n, 1, 1, 1)
                    for s in range(2):
                        anchor = be.augment_masked(x, units[s], zeros, *reference, m, **opt)
                        assert torch.equal(bits(got["stains"][s])[pick], bits(anchor)[pick]), (tag, s)
                        # ... and a tile without an estimate is background in the separation, copied in the augmentation
                        assert (bits(got["stains"][s])[~has] == bits(level.reshape(1))[0]).all(), (tag, s)
            # values under the mask do not matter: NaN and Inf there change no output bit and no estimate row
            if dt != torch.uint8:
                for fill in (float("nan"), float("inf"), float("-inf")):
                    y = torch.where(where, x, torch.full_like(x, fill))
                    want = be.separate_masked(x, *ref, m, concentrations=True)
                    again = be.separate_masked(y, *ref, m, concentrations=True)
                    assert_same_separation(again, want, (what, mask_name, fill))
                    assert same_bits(again["he"], want["he"]) and same_bits(again["max_c"], want["max_c"])
                    given = be.separate_apply_masked(y, est["he"], est["max_c"], None, None, m, concentrations=True)
                    assert_same_separation(given, be.separate_apply_masked(x, est["he"], est["max_c"], None, None, m, concentrations=True), (what, mask_name, fill, "own"))


def test_unaligned_pointers_at_the_c_abi(dev, be, ref):
    """Images, mask, stain images and concentrations one element off a 16-byte address, each on its own: the scalar path, the same bits."""
    lib = _native.require()
    sm, tmc = ref
    stream = _native.stream_ptr(dev)
    for dt in (torch.float32, torch.uint8, torch.bfloat16):
        tiles = synth.he_batch(2, 96, 96, seed0=77)
        x = synth.as_dtype(tiles, dt).to(dev)
        n, _, h, w = x.shape
        assert h * w > work_item_pixels(dt, dt, vector=False)
        m = mask_t(mm.blocks(n, h, w, 5), dev)
        est = be.estimate_masked(x, m)
        want = be.separate_apply_masked(x, est["he"], est["max_c"], sm, tmc, m, concentrations=True)
        code = _native.DTYPE_CODES[dt]
        for moved in ("none", "images", "mask", "stains", "conc"):
            xs = unaligned_copy(x) if moved == "images" else x
            ms = unaligned_copy(m) if moved == "mask" else m
            stains = unaligned_copy(torch.zeros_like(want["stains"])) if moved == "stains" else torch.zeros_like(want["stains"])
            conc = unaligned_copy(torch.zeros_like(want["concentrations"])) if moved == "conc" else torch.zeros_like(want["concentrations"])
            rc = lib.sx_macenko_separate_apply_masked(xs.data_ptr(), stains.data_ptr(), conc.data_ptr(), code, n, h, w, est["he"].data_ptr(), est["max_c"].data_ptr(), n,
                                                      sm.data_ptr(), tmc.data_ptr(), ms.data_ptr(), 0, stream)
            assert rc == _native.SX_OK, _native.last_error()
            assert same_bits(stains, want["stains"]) and same_bits(conc, want["concentrations"]), (dt, moved)
            # the unmasked call and the sequenced one through the same pointers
            if moved != "mask":
                plain = be.separate_apply(x, est["he"], est["max_c"], sm, tmc, concentrations=True)
                rc = lib.sx_macenko_separate_apply(xs.data_ptr(), stains.data_ptr(), conc.data_ptr(), code, n, h, w, est["he"].data_ptr(), est["max_c"].data_ptr(), n,
                                                   sm.data_ptr(), tmc.data_ptr(), 0, stream)
                assert rc == _native.SX_OK, _native.last_error()
                assert same_bits(stains, plain["stains"]) and same_bits(conc, plain["concentrations"]), (dt, moved, "unmasked")
            ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, n, h, w, CLASSIC)), dtype=torch.uint8, device=dev)
            rc = lib.sx_macenko_separate_masked(xs.data_ptr(), stains.data_ptr(), conc.data_ptr(), code, n, h, w, ms.data_ptr(), sm.data_ptr(), tmc.data_ptr(), None, None, 0,
                                                ws.data_ptr(), ws.numel(), stream)
            assert rc == _native.SX_OK, _native.last_error()
            assert same_bits(stains, want["stains"]) and same_bits(conc, want["concentrations"]), (dt, moved, "sequenced")
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. against the restatement
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_against_the_restatement(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    x8, rule = real[0][:5], real[1][:5]
    x = synth.as_dtype(x8, dt)
    xn = mn.oracle_input(x)
    sm, tmc = ref
    tmcn = tmc.cpu().numpy()
    for mask_name, mask in (("rule", rule), ("disc", mm.disc(5, 256, 256)), ("blocks", mm.blocks(5, 256, 256, 16))):
        m = mask_t(mask, dev)
        rows = mm.estimate(xn, mask, signs="positive_sum")
        est = be.estimate_masked(x.to(dev), m)
        check_rows(est, rows, f"{mask_name} {name}")
        where = inside(mask, x)
        for reference in ((None, None), ref):
            normalised = reference[0] is not None
            got = be.separate_masked(x.to(dev), *reference, m, concentrations=True, max_conc=True)
            assert same_bits(got["he"], est["he"]) and same_bits(got["max_c"], est["max_c"])
            he, max_c = got["he"].cpu().numpy(), got["max_c"].cpu().numpy()
            conc, levels = sn.separate(xn, mask, he, max_c, (sm.cpu().numpy(), tmcn) if normalised else None)
            err = np.abs(got["concentrations"].cpu().numpy() - conc)
            measured = []
            for i in range(5):
                for s in range(2):
                    bound = TOL_CONC * (max(1.0, float(tmcn[s] / max_c[i, s])) if normalised else 1.0)
                    worst = float(err[i, s][mask[i]].max())
                    measured.append((worst / bound, worst, bound, i, s))
            share, worst, bound, i, s = max(measured)
            print(f"{mask_name} {name} normalised={normalised}: max |C' - restated| on masked-in pixels, nearest its bound: {worst:.3e} (bound {bound:.3e}; tile {i}, stain {s})")
            assert share <= 1.0, (mask_name, i, s, worst, bound)
            for s in range(2):
                check_output(got["stains"][s], levels[s], where, dt, f"{mask_name} {name} normalised={normalised} stain {s}")


# ------------------------------------------------------------------------------------------------ 4. it matters
def test_the_mask_matters_for_the_concentrations_of_a_sparse_tile(dev, ref, real):
    """Real crop 4, a third tissue: the normalised concentrations of the tissue have their 99th percentile at target_max_conc when the
    normaliser separates under its rule, and at least 15 % above it when maxC is taken over all pixels."""
    sm, tmc = ref
    x = synth.as_dtype(real[0][4:5], torch.float32).to(dev)
    norm = Macenko(device=dev, mask="luminosity")
    norm._stain_matrix, norm._target_max_conc, norm._is_fitted = sm, tmc, True
    plain = Macenko(device=dev)
    plain._stain_matrix, plain._target_max_conc, plain._is_fitted = sm, tmc, True
    made, _ = tissue_mask(x, 0.8)
    tissue = made[0].cpu().numpy().astype(bool).reshape(-1)
    masked, unmasked = norm.separate(x, stains=False, concentrations=True), plain.separate(x, stains=False, concentrations=True)
    tmcn = tmc.cpu().numpy().astype(np.float64)
    for s in range(2):
        at = float(so.nearest_rank(masked.concentrations[0, s].cpu().numpy().reshape(-1)[tissue], 99))
        over = float(so.nearest_rank(unmasked.concentrations[0, s].cpu().numpy().reshape(-1)[tissue], 99))
        bound = TOL_CONC * max(1.0, float(tmcn[s] / float(masked.max_concentrations[0, s])))
        print(f"crop 4 stain {s}: 99th percentile of the tissue's C' masked {at:.6f} (tmc {tmcn[s]:.6f}, bound {bound:.2e}), unmasked {over:.6f} = {over / tmcn[s]:.3f} tmc")
        assert abs(at - tmcn[s]) <= bound, (s, at)
        assert over >= 1.15 * tmcn[s], (s, over)


# ------------------------------------------------------------------------------------------------ 5. degenerate groups
def test_degenerate_groups(dev, be, ref, real):
    sm, tmc = ref
    x8 = torch.cat([real[0][[5, 3]], synth.background_stripes(synth.he_batch(3, 256, 256))[1:]])      # glass crop, tissue crop, half glass, all glass
    for dt in (torch.uint8, torch.float32):
        x = synth.as_dtype(x8, dt).to(dev)
        n, _, h, w = x.shape
        level = no_stain_level(dt, False).to(dev)
        for what, mask, has in (("zeros", mm.zeros(n, h, w), False), ("two", mm.exactly(n, h, w, 2), False), ("three", mm.exactly(n, h, w, 3), True)):
            m = mask_t(mask, dev)
            for reference in ((None, None), ref):
                got = be.separate_masked(x, *reference, m, concentrations=True, max_conc=True)
                if not has:
                    assert torch.isnan(got["he"]).all() and torch.isnan(got["max_c"]).all(), what
                    assert (got["stains"] == level).all() and (got["concentrations"].view(torch.int32) == 0).all(), what
                else:
                    assert torch.isfinite(got["he"]).all(), what
                    where = torch.from_numpy(inside(mask, x).copy()).to(dev)
                    assert (got["stains"][0][~where] == level).all() and (got["concentrations"].view(torch.int32)[~where[:, :2]] == 0).all(), what
        # a NaN source row makes the tile background whatever the mask says; the other tiles are those of the call without it
        made, counts = tissue_mask(x, 0.8)
        est = be.estimate_masked(x, made)
        empty = (counts < 3)
        assert bool(empty[0]) and bool(empty[3]) and not bool(empty[1]) and not bool(empty[2])
        ones = torch.ones_like(made)
        for reference in ((None, None), ref):
            got = be.separate_apply_masked(x, est["he"], est["max_c"], *reference, ones, concentrations=True)
            assert (got["stains"][:, empty] == level).all() and (got["concentrations"][empty].view(torch.int32) == 0).all()
            assert not torch.isnan(got["stains"].float()).any() and not torch.isnan(got["concentrations"]).any()
            alone = be.separate_apply_masked(x[1:3].contiguous(), est["he"][1:3].contiguous(), est["max_c"][1:3].contiguous(), *reference, ones[1:3].contiguous(), concentrations=True)
            assert same_bits(alone["stains"], got["stains"][:, 1:3]) and same_bits(alone["concentrations"], got["concentrations"][1:3])
            # ... and a tile's result under the rule does not depend on its batch neighbours
            batch = be.separate_masked(x, *reference, made, concentrations=True)
            one = be.separate_masked(x[1:2].contiguous(), *reference, made[1:2].contiguous(), concentrations=True)
            assert same_bits(one["stains"], batch["stains"][:, 1:2]) and same_bits(one["concentrations"], batch["concentrations"][1:2])
            shuffled = be.separate_masked(x[[2, 0, 1]].contiguous(), *reference, made[[2, 0, 1]].contiguous(), concentrations=True)
            assert same_bits(shuffled["stains"][:, 2:3], one["stains"])


# ------------------------------------------------------------------------------------------------ 6. plumbing
def test_poisoned_workspace_side_stream_and_graph(dev, be, ref, real):
    sm, tmc = ref
    x8, rule = real
    x = synth.as_dtype(x8[:4], torch.float32).to(dev)
    x2 = synth.as_dtype(x8[[3, 2, 1, 0]], torch.float32).to(dev)
    m, m2 = mask_t(rule[:4], dev), mask_t(mm.blocks(4, 256, 256, 16, seed=8), dev)
    want, want2 = be.separate_masked(x, sm, tmc, m, concentrations=True), be.separate_masked(x2, sm, tmc, m2, concentrations=True)
    est, est2 = be.estimate_masked(x, m), be.estimate_masked(x2, m2)
    # a workspace poisoned beforehand changes nothing
    for fill in (0xFF, 0x7F):
        be.last_workspace.fill_(fill)
        again = be.separate_masked(x, sm, tmc, m, concentrations=True)
        assert_same_separation(again, want, ("poisoned", fill))
        assert same_bits(again["he"], want["he"]) and same_bits(again["max_c"], want["max_c"])
    # a side stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = be.separate_masked(x, sm, tmc, m, concentrations=True)
        given = be.separate_apply_masked(x, est["he"], est["max_c"], sm, tmc, m, concentrations=True)
    side.synchronize()
    assert_same_separation(on_side, want, "side stream")
    assert_same_separation(given, want, "side stream, given")
    # a captured call: one chain on one stream, replayed after new images, mask bytes and source rows were copied into the same buffers
    xbuf, mbuf, he_buf, mc_buf = x.clone(), m.clone(), est["he"].clone(), est["max_c"].clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        be.separate_masked(xbuf, sm, tmc, mbuf, concentrations=True)      # (warm-up on the capture stream: its workspace exists before the capture)
        be.separate_apply_masked(xbuf, he_buf, mc_buf, sm, tmc, mbuf, concentrations=True)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap_given = be.separate_apply_masked(xbuf, he_buf, mc_buf, sm, tmc, mbuf, concentrations=True)
            cap_own = be.separate_masked(xbuf, sm, tmc, mbuf, concentrations=True)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_separation(cap_given, want, "graph, given")
    assert_same_separation(cap_own, want, "graph")
    xbuf.copy_(x2)
    mbuf.copy_(m2)
    he_buf.copy_(est2["he"])
    mc_buf.copy_(est2["max_c"])
    graph.replay()
    torch.cuda.synchronize()
    assert_same_separation(cap_given, want2, "graph replayed, given")
    assert_same_separation(cap_own, want2, "graph replayed")
    assert same_bits(cap_own["he"], est2["he"])


def test_c_abi_argument_errors_enqueue_nothing_and_a_raw_call_works(dev, be, ref):
    lib = _native.require()
    sm, tmc = ref
    x = synth.as_dtype(synth.he_batch(2, 64, 64), torch.float32).to(dev)
    m = torch.ones(2, 64, 64, dtype=torch.uint8, device=dev)
    stains, conc = torch.full((2, 2, 3, 64, 64), -7.0, device=dev), torch.full((2, 2, 64, 64), -7.0, device=dev)
    est = be.estimate(x)
    he, mc = est["he"], est["max_c"]
    code = _native.DTYPE_CODES[torch.float32]
    ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, 2, 64, 64, CLASSIC)), dtype=torch.uint8, device=dev)
    stream = _native.stream_ptr(dev)
    BAD = _native.SX_ERR_BAD_ARG

    def given(st=stains.data_ptr(), c=conc.data_ptr(), h=he.data_ptr(), k=mc.data_ptr(), n_sources=2, s=sm.data_ptr(), t=tmc.data_ptr(), flags=0):
        return lib.sx_macenko_separate_apply(x.data_ptr(), st, c, code, 2, 64, 64, h, k, n_sources, s, t, flags, stream)

    def given_masked(st=stains.data_ptr(), c=conc.data_ptr(), h=he.data_ptr(), k=mc.data_ptr(), n_sources=2, s=sm.data_ptr(), t=tmc.data_ptr(), mask=m.data_ptr(), flags=0):
        return lib.sx_macenko_separate_apply_masked(x.data_ptr(), st, c, code, 2, 64, 64, h, k, n_sources, s, t, mask, flags, stream)

    def own_masked(st=stains.data_ptr(), c=conc.data_ptr(), s=sm.data_ptr(), t=tmc.data_ptr(), mask=m.data_ptr(), flags=0):
        return lib.sx_macenko_separate_masked(x.data_ptr(), st, c, code, 2, 64, 64, mask, s, t, None, None, flags, ws.data_ptr(), ws.numel(), stream)

    for call in (given_masked, own_masked):
        assert call(mask=None) == BAD and _native.last_error(lib)
        assert call(flags=_native.MACENKO_CHANNELS_LAST) == BAD and call(flags=_native.MACENKO_SAMPLED) == BAD
    for call in (given, given_masked, own_masked):
        assert call(st=None, c=None) == BAD      # both outputs NULL
        assert call(s=None) == BAD and call(t=None) == BAD      # one of the reference pair
    for call in (given, given_masked):
        assert call(n_sources=0) == BAD and call(n_sources=3) == BAD
        assert call(h=None) == BAD and call(k=None) == BAD      # no source; normalise mode without source_max_c
    assert given(flags=_native.MACENKO_SAMPLED) == BAD
    torch.cuda.synchronize()
    assert (stains == -7.0).all() and (conc == -7.0).all()
    # successful raw calls: all three agree under an all-ones mask, own basis without source_max_c included
    want = be.separate(x, sm, tmc, concentrations=True)
    for call in (given, given_masked, own_masked):
        stains.fill_(-7.0)
        conc.fill_(-7.0)
        assert call(flags=CLASSIC) == _native.SX_OK, _native.last_error(lib)
        assert same_bits(stains, want["stains"]) and same_bits(conc, want["concentrations"]), call.__name__
    own = be.separate(x, concentrations=True)
    assert given(k=None, s=None, t=None) == _native.SX_OK and same_bits(stains, own["stains"]) and same_bits(conc, own["concentrations"])
    assert given(st=None) == _native.SX_OK and given(c=None) == _native.SX_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. the public method
def test_public_method(dev, be, ref, real):
    sm, tmc = ref
    x = real[0][:5].to(dev)
    norm = Macenko(device=dev)
    norm._stain_matrix, norm._target_max_conc, norm._is_fitted = sm, tmc, True
    slide = norm.estimate(x, pooled=True)      # one basis for the slide
    assert isinstance(slide, StainEstimate) and slide.stain_matrices.shape == (1, 3, 2)
    got = norm.separate(x, source=slide, concentrations=True)
    want = be.separate_apply(x, slide.stain_matrices, slide.max_concentrations, sm, tmc, concentrations=True)
    assert same_bits(got.hematoxylin, want["stains"][0]) and same_bits(got.eosin, want["stains"][1]) and same_bits(got.concentrations, want["concentrations"])
    assert got.stain_matrices.shape == (5, 3, 2) and got.max_concentrations.shape == (5, 2) and same_bits(got.stain_matrices[4], slide.stain_matrices[0])
    # a pair, a StainSeparation and per-tile rows are sources too; own basis keeps the source's vectors
    per_tile = norm.separate(x, concentrations=True)
    again = norm.separate(x, source=per_tile, concentrations=True)
    assert same_bits(again.hematoxylin, per_tile.hematoxylin) and same_bits(again.concentrations, per_tile.concentrations)
    own = norm.separate(x, source=(slide.stain_matrices[0], None), own_basis=True)
    assert same_bits(own.eosin, be.separate_apply(x, slide.stain_matrices, None)["stains"][1]) and own.max_concentrations is None
    # the normaliser's rule: separate goes through it, as fit / transform / estimate / apply do
    ruled = Macenko(device=dev, mask="luminosity")
    ruled._stain_matrix, ruled._target_max_conc, ruled._is_fitted = sm, tmc, True
    made = tissue_mask(x, 0.8)[0]
    by_rule, by_mask = ruled.separate(x, concentrations=True), norm.separate(x, mask=made, concentrations=True)
    assert same_bits(by_rule.hematoxylin, by_mask.hematoxylin) and same_bits(by_rule.concentrations, by_mask.concentrations)
    assert same_bits(by_rule.stain_matrices, by_mask.stain_matrices) and same_bits(norm.separate(x, mask="luminosity").eosin, by_rule.eosin)
    assert not same_bits(by_rule.concentrations, per_tile.concentrations)
    masked_slide = ruled.separate(x, source=slide, concentrations=True)
    backend = be.separate_apply_masked(x, slide.stain_matrices, slide.max_concentrations, sm, tmc, made, concentrations=True)
    assert same_bits(masked_slide.hematoxylin, backend["stains"][0]) and same_bits(masked_slide.concentrations, backend["concentrations"])
    assert (masked_slide.concentrations[(made == 0)[:, None].expand(5, 2, 256, 256)] == 0).all()
