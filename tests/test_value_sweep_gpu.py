"""Every input value through the per-pixel kernels, against float64 (the sets and the reference: tests/_value_sweep.py; what they rely on:
tests/test_value_sweep_cpu.py).  The entry points are the element-wise ones of the public classes -- ``HistogramMatching.estimate`` /
``apply``, ``tissue_mask``, ``Reinhard.apply`` / ``estimate``, ``Macenko.apply`` -- which take their statistics as arguments, so nothing
ill-posed stands between a value and its result.

* Histogram matching is exact arithmetic: counts and looked-up pixels are compared bit for bit, non-finite values included (+Inf -> 255,
  -Inf -> 0, the reference's clamp; NaN -> bin 0, the library's rule where the reference's cast is undefined).
* The tissue rule equals the float64 rule outside the band of tests/_masked_numpy.py; a pixel with a NaN member is background.
* Reinhard and Macenko with GIVEN statistics: inside the domain |out - float64| <= the project's bound (1e-4 on [0, 1]; TOL_255 on 0-255)
  for float32, plus half an ulp of the output type at the reference value for bf16 / f16; uint8 equals the truncated float64 value except
  within the bound of an integer, where one level is allowed.  Outside the domain -- finite or not -- every output is finite and in range,
  and replacing those pixels by 0.5 grey changes no bit of any other pixel (no NaN through a pack, a ballot or an MFMA block).
* The 8-bit code gates mark whole tiles: tiles of k / 255 beside tiles whose every element, or whose one element, is k / 255 +- 1 ulp (or
  -0.0) -- the transform (which codes the tiles that pass) gives the bits of estimate + apply (which never codes); so do separation and
  augmentation with the tile's own estimate against the same call with that estimate given.
* The stain kernels (separation, jitter, deconvolution, quantify, luminosity apply): tests/test_value_sweep_stains_gpu.py.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import HistogramMatching, Macenko, MacenkoAugment, Reinhard, StainEstimate, synth, tissue_mask
from tests import _hm_slide_numpy as sn
from tests import _masked_numpy as mn
from tests import _value_sweep as vs
from tests.test_apply_gpu import TOL_255
from tests.test_hm_slide_gpu import bits, same_bits, unaligned_copy

pytestmark = pytest.mark.gpu

SETS = {"A": vs.set_a, "B_bf16": lambda: vs.set_b(torch.bfloat16), "B_f16": lambda: vs.set_b(torch.float16), "C": vs.set_c}
MEAN_ATOL, STD_RTOL, STD_ATOL = 2e-3, 1e-4, 1e-3      # LAB statistics: the project's bounds (tests/test_per_tile_gpu.py, test_tissue_mask_gpu.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def forms(x: torch.Tensor):
    yield "aligned", x
    yield "unaligned", unaligned_copy(x)


def tile_counts(levels: np.ndarray, mask: np.ndarray | None = None) -> np.ndarray:
    """(N, 3, 256) int64 bincounts of (N, 3, H, W) uint8 levels, over the pixels of ``mask`` (N, H, W) where given."""
    n = levels.shape[0]
    key = (np.arange(n * 3, dtype=np.int64).reshape(n, 3, 1, 1) << 8) + levels
    if mask is not None:
        key = key[np.broadcast_to(mask[:, None], levels.shape)]
    return np.bincount(key.reshape(-1), minlength=n * 3 * 256).reshape(n, 3, 256).astype(np.int64)


# ------------------------------------------------------------------------------------------------ histogram matching: exact
@pytest.mark.parametrize("name", list(SETS))
def test_histogram_estimate_counts_every_value_bit_for_bit(dev, name):
    sweep = SETS[name]()
    for layout in sweep.layouts.values():
        levels = sweep.spread(layout, sweep.levels)
        want = torch.from_numpy(tile_counts(levels))
        n, pixels = layout.n, layout.h * layout.w
        for last in (False, True):
            axis = -1 if last else 1
            norm = HistogramMatching(device=dev, backend="torch_hip", channel_axis=axis)
            for form, x in forms(sweep.images(layout, channels_last=last).to(dev)):
                where = (name, layout.name, axis, form)
                per_tile, pooled = norm.estimate(x), norm.estimate(x, pooled=True)
                assert torch.equal(per_tile.counts.cpu(), want), where
                assert torch.equal(per_tile.pixels.cpu(), torch.full((n,), pixels, dtype=torch.int64)), where
                assert torch.equal(per_tile.counts.sum(2).cpu(), torch.full((n, 3), pixels, dtype=torch.int64)), where
                assert torch.equal(pooled.counts.cpu(), want.sum(0, keepdim=True)) and pooled.pixels.cpu().tolist() == [n * pixels], where
                assert norm._get_backend_impl().workspace_status() == 0, where
                # the masked estimate counts the tissue of the rule (held to float64 in the rule test below), every member with its pixel
                mask, tissue = tissue_mask(x, norm.luminosity_threshold, channel_axis=axis)
                want_tissue = torch.from_numpy(tile_counts(levels, mask.cpu().numpy() != 0))
                per_tile, pooled = norm.estimate(x, mask="luminosity"), norm.estimate(x, pooled=True, mask="luminosity")
                assert torch.equal(per_tile.counts.cpu(), want_tissue) and torch.equal(per_tile.pixels, tissue), where
                assert torch.equal(per_tile.counts.sum(2), tissue[:, None].expand(n, 3)), where
                assert torch.equal(pooled.counts.cpu(), want_tissue.sum(0, keepdim=True)) and pooled.pixels.item() == int(tissue.sum()), where
                assert norm._get_backend_impl().workspace_status() == 0, where
        print(f"{name} {layout.name}: {n} x {layout.h} x {layout.w}: counts equal the float32 gate's, bins 0 / 255 hold {want[:, 0, 0].sum().item()} / {want[:, 0, 255].sum().item()} of channel 0")


@pytest.mark.parametrize("name", list(SETS))
def test_histogram_apply_with_foreign_tables_bit_for_bit(dev, name):
    sweep = SETS[name]()
    luts = vs.monotone_tables()
    tables = torch.from_numpy(luts).to(dev)
    for layout in sweep.layouts.values():
        for last in (False, True):
            axis = -1 if last else 1
            norm = HistogramMatching(device=dev, backend="torch_hip", channel_axis=axis)
            ref = synth.as_dtype(synth.reference_tile(64, 64), sweep.dtype)
            norm.fit((ref.permute(0, 2, 3, 1).contiguous() if last else ref).to(dev))
            src = sweep.images(layout, channels_last=last)
            images = mn.oracle_input(src)
            if images.dtype != np.uint8:
                images = np.where(np.isnan(images), np.float32(0), images)      # (the library's NaN rule, see vs.grey_levels)
            with np.errstate(invalid="ignore", over="ignore"):
                want = mn.oracle_cast(sn.lookup(images, luts, axis), sweep.dtype)
            for form, x in forms(src.to(dev)):
                got = norm.apply(x, tables)
                assert same_bits(got.cpu(), want), (name, layout.name, axis, form, int((bits(got.cpu()) != bits(want)).sum()))


# ------------------------------------------------------------------------------------------------ the tissue rule
@pytest.mark.parametrize("name", list(SETS))
def test_tissue_rule_is_the_float64_rule_outside_the_band(dev, name):
    sweep = SETS[name]()
    has_nan = np.isnan(sweep.x32).any(axis=1)
    for threshold in vs.THRESHOLDS:
        tissue_px, decided_px = sweep.rule(threshold, mn.L_BAND)
        for layout in sweep.layouts.values():
            tissue, decided, nan = (sweep.spread(layout, a) for a in (tissue_px, decided_px, has_nan))
            for last in (False, True):
                for form, x in forms(sweep.images(layout, channels_last=last).to(dev)):
                    mask, counts = tissue_mask(x, threshold, channel_axis=-1 if last else 1)
                    m = mask.cpu().numpy()
                    assert set(np.unique(m).tolist()) <= {0, 1}
                    wrong = int(((m != 0) != tissue)[decided].sum())
                    assert wrong == 0, (name, threshold, layout.name, last, form, wrong)
                    assert not m[nan].any(), "a pixel with a NaN member is background"
                    assert torch.equal(counts.cpu(), torch.from_numpy(m.reshape(layout.n, -1).sum(axis=1).astype(np.int64)))
            print(f"{name} threshold {threshold} {layout.name}: the float64 rule on {int(decided.sum())} decided pixels ({int((~decided).sum())} in the band, {int(nan.sum())} with a NaN)")


# ------------------------------------------------------------------------------------------------ Reinhard and Macenko with given statistics
def reinhard_normaliser(dev):
    st = vs.statistics()
    norm = Reinhard(device=dev, backend="torch_hip")
    norm._reference_mean, norm._reference_std = torch.from_numpy(st["ref_mean"]).to(dev), torch.from_numpy(st["ref_std"]).to(dev)      # the oracle's fit, not the GPU's
    norm._is_fitted = True
    return norm, (torch.from_numpy(st["mean"]).to(dev), torch.from_numpy(st["std"]).to(dev))


def macenko_normaliser(dev):
    st = vs.statistics()
    norm = Macenko(device=dev, backend="torch_hip")
    norm._stain_matrix, norm._target_max_conc = torch.from_numpy(st["sm"]).to(dev), torch.from_numpy(st["tmc"]).to(dev)
    norm._is_fitted = True
    return norm, StainEstimate(torch.from_numpy(st["he"]).reshape(1, 3, 2).to(dev), torch.from_numpy(st["max_c"]).reshape(1, 2).to(dev), None)


def check_against_float64(what, sweep, layout, out: torch.Tensor, ref_px: np.ndarray, raw_px: np.ndarray, dom_px: np.ndarray, bound: float, top: float) -> float:
    """``out`` (N, 3, H, W) of the sweep's type against the float64 reference on its scale 0..``top`` (1 or 255); returns the worst error."""
    assert out.dtype == sweep.dtype and tuple(out.shape) == (layout.n, 3, layout.h, layout.w), what
    dom = np.broadcast_to(sweep.spread(layout, dom_px)[:, None], out.shape)
    ref = sweep.spread(layout, ref_px)
    if sweep.dtype == torch.uint8:      # the float64 value on the 0-255 scale, truncated; one level either way within the bound of an integer
        got = out.cpu().numpy().astype(np.int16)
        to_levels = 255.0 / top
        near = vs.near_integer(sweep.spread(layout, raw_px) * to_levels, bound * to_levels)
        want = np.trunc(ref * to_levels).astype(np.int16)
        strict = dom & ~near
        assert np.array_equal(got[strict], want[strict]), (what, int((got != want)[strict].sum()))
        worst = int(np.abs(got - want)[dom & near].max(initial=0))
        assert worst <= 1, (what, worst)
        print(f"{what}: uint8 equals trunc(float64) on {int(strict.sum())} elements; {int((got != want)[dom & near].sum())} of {int((dom & near).sum())} within {bound * to_levels:.3e} of an integer differ, by one level")
        return float(worst)
    got = out.cpu().double().numpy()
    # outside the domain, finite or not: a finite value of the output range
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= top, (what, "out of range")
    with np.errstate(invalid="ignore"):
        allowed = bound + (vs.half_ulp(ref, sweep.dtype) if sweep.dtype != torch.float32 else 0.0)
        err = np.where(dom, np.abs(got - ref), 0.0)
        over = np.where(dom, err - allowed, -1.0)
    worst = float(err.max())
    print(f"{what}: max |out - float64| = {worst:.3e} on {int(dom.sum())} in-domain elements (bound {bound:.3e}" + ("" if sweep.dtype == torch.float32 else " + half an ulp") + f"), worst excess {float(over.max()):.3e}")
    assert float(over.max()) <= 0.0, (what, worst)
    return worst


def sweep_an_apply(dev, name, kind):
    sweep = SETS[name]()
    if kind == "reinhard":
        (norm, source), refs, dom_px, bound, top = reinhard_normaliser(dev), sweep.reinhard, sweep.reinhard_domain, vs.REINHARD_TOL, 1.0
    else:
        (norm, source), refs, dom_px, bound, top = macenko_normaliser(dev), sweep.macenko, sweep.macenko_domain, TOL_255, 255.0
    for layout in sweep.layouts.values():
        dom = torch.from_numpy(np.broadcast_to(sweep.spread(layout, dom_px)[:, None], (layout.n, 3, layout.h, layout.w)).copy())
        clean = sweep.images(layout, replace=~dom_px).to(dev)
        for form, x in forms(sweep.images(layout).to(dev)):
            what = f"{kind} {name} {layout.name} {form}"
            out = norm.apply(x, source)
            check_against_float64(what, sweep, layout, out, refs["out"], refs["raw"], dom_px, bound, top)
            # independence: the out-of-domain pixels replaced by 0.5 grey -- every other pixel keeps its bits
            if not bool(dom.all()):
                again = norm.apply(clean if form == "aligned" else unaligned_copy(clean), source)
                assert torch.equal(bits(out.cpu())[dom], bits(again.cpu())[dom]), (what, "a pixel outside the domain changed another pixel")
                assert torch.isfinite(again.float()).all()


@pytest.mark.parametrize("name", list(SETS))
def test_reinhard_apply_against_float64(dev, name):
    sweep_an_apply(dev, name, "reinhard")


@pytest.mark.parametrize("name", list(SETS))
def test_macenko_apply_against_float64(dev, name):
    sweep_an_apply(dev, name, "macenko")


@pytest.mark.parametrize("name", list(SETS))
def test_reinhard_estimate_against_float64(dev, name):
    """The LAB statistics of the in-domain tiles (pixels outside the domain replaced by 0.5 grey; set A as it is), per tile and pooled."""
    sweep = SETS[name]()
    norm, _ = reinhard_normaliser(dev)
    outside = ~sweep.reinhard_domain
    for layout in sweep.layouts.values():
        lab = sweep.spread(layout, sweep.reinhard["lab"], replace=outside).transpose(0, 2, 3, 1).reshape(layout.n, -1, 3)
        x = sweep.images(layout, replace=outside).to(dev)
        for form, x in forms(x):
            for pooled in (False, True):
                rows = lab.reshape(1, -1, 3) if pooled else lab
                want_mean, want_std = rows.mean(axis=1), rows.std(axis=1, ddof=1)
                got = norm.estimate(x, pooled=pooled)
                mean, std = got.mean.cpu().double().numpy(), got.std.cpu().double().numpy()
                assert mean.shape == want_mean.shape and std.shape == want_std.shape
                d_mean, d_std = np.abs(mean - want_mean), np.abs(std - want_std)
                print(f"estimate {name} {layout.name} {form} {'pooled' if pooled else 'per tile'}: max |mean - float64| = {d_mean.max():.3e} (bound {MEAN_ATOL}), max |std - float64| = {d_std.max():.3e} "
                      f"(bound {STD_ATOL} + {STD_RTOL} std)")
                assert (d_mean <= MEAN_ATOL).all() and (d_std <= STD_ATOL + STD_RTOL * np.abs(want_std)).all()


# ------------------------------------------------------------------------------------------------ the 8-bit code gates
def test_code_gates_take_no_neighbour_of_a_grey_level_for_a_code(dev):
    """vs.gate_tiles(): float32, 2^20 pixels, H * W % 4 == 0 -- the batch both transforms run coded.  Tiles of grey levels, which the gates
    pass, beside tiles in which EVERY element is one ulp off its level and tiles of grey levels but for ONE element (one ulp up, one ulp
    down, -0.0 for 0; first pack, last pack, a lane in the middle of a wave).  The gates mark a whole tile, so only such tiles can show
    what they make of a neighbour: a gate that took k / 255 +- 1 ulp for level k would code the tile and return table[k] where estimate +
    apply (given statistics, no gate, never coded) evaluates f(k / 255 +- 1 ulp).  The transform equals estimate + apply bit for bit on
    every tile.  So do ``Macenko.separate(x)`` (its last pass reads the codes of the tiles the first pass coded) against
    ``separate(x, source=estimate(x))`` and the ``MacenkoAugment`` forward (the transform's passes in front of its own reconstruct pass)
    against estimate + apply with the same factors, both in their own basis and normalised: one launch with a given basis has no gate.

    Measured with the bit comparison of both gates replaced by |x - k / 255| <= 3e-7 in a scratch build: the test fails -- Reinhard with
    batch statistics differs on all 16 tiles (the pooled statistics move), Reinhard with tile statistics and Macenko on 6 each: the three
    ``all`` tiles and the ``up`` tile of every spot.  A single element moved DOWN came out with table[k]'s bits by chance in those two, and
    -0.0 evaluates to what 0 does in both transforms, so those tiles can show a loose gate only through the statistics."""
    images, tiles = vs.gate_tiles()
    n, h, w = vs.GATE_SHAPE
    assert tuple(images.shape) == (n, 3, h, w) and n * h * w >= 1 << 20 and (h * w) % 4 == 0 and images.dtype == torch.float32
    x = images.to(dev)
    reinhard, _ = reinhard_normaliser(dev)
    macenko, _ = macenko_normaliser(dev)
    cases = {}
    for statistics in ("batch", "tile"):
        reinhard.statistics = statistics
        cases[f"Reinhard, {statistics} statistics"] = (reinhard.transform(x), reinhard.apply(x, reinhard.estimate(x, pooled=statistics == "batch")))
    estimate = macenko.estimate(x)
    cases["Macenko"] = (macenko.transform(x), macenko.apply(x, estimate))
    # separation and augmentation with each tile's OWN estimate (the forms that may code a tile) against the same call with that estimate
    # GIVEN (one launch, no gate, never coded).  Whether or not a form has a coded path, the comparison holds and costs one call.
    for own_basis in (True, False):
        mode = "own basis" if own_basis else "normalised"
        own = macenko.separate(x, own_basis=own_basis, stains=True, concentrations=True)
        given = macenko.separate(x, source=estimate, own_basis=own_basis, stains=True, concentrations=True)
        for part in ("hematoxylin", "eosin", "concentrations"):
            cases[f"Macenko.separate, {mode}, {part}"] = (getattr(own, part), getattr(given, part))
    pairs = torch.tensor(vs.JITTER, dtype=torch.float32)[torch.arange(n) % len(vs.JITTER)].to(dev)      # (N, 2 (alpha, beta), 2)
    alpha, beta = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    augment = MacenkoAugment(normalizer=macenko, device=dev, normalize_to_0_1=False)
    cases["MacenkoAugment, normalised"] = (augment(x, alpha, beta), macenko.apply(x, estimate, alpha=alpha, beta=beta))
    cases["MacenkoAugment, own basis"] = (MacenkoAugment(device=dev, normalize_to_0_1=False)(x, alpha, beta), macenko.apply(x, estimate, alpha=alpha, beta=beta, own_basis=True))
    differ ={what: sorted(name for name, t in tiles.items() if not same_bits(got[t], want[t])) for what, (got, want) in cases.items()}
    for what, names in differ.items():
        print(f"code gates, {what}: transform != estimate + apply on {len(names)} of {n} tiles {names}")
    assert not any(differ.values()), differ
