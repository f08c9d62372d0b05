"""The value-domain sweeps before a GPU is involved (tests/_value_sweep.py): the float64 reference against the float32 oracle, and the
conditions the GPU file (tests/test_value_sweep_gpu.py) relies on.

1. On sets A-C inside the domains the float32 oracle stays within a QUARTER of the project's parity bound of the float64 reference --
   1e-4 / 4 on [0, 1] for Reinhard, TOL_255 / 4 on 0-255 for Macenko, no exclusions -- so that three quarters of each bound are the
   kernel's.  (The Reinhard domain stops at 2 because the oracle's own float32 error grows with |x|: 1.8e-5 on [-1, 2], 8.6e-5 by 16.)
   One domain had to be narrowed: the random triples of set C are held to [-1/4, 5/4] per member for Reinhard, because the float32 oracle
   itself is 4.1e-5 from float64 on triples of [-1, 2] (tests/_value_sweep.py: Sweep.reinhard_domain); the bound stays.
2. Every piecewise function takes both of its branches on at least 1000 in-domain pixels of each float set.
3. The pixels left out of rule comparisons (float64 L within L_BAND of the cut) are at most BORDER_CAP of every set, thresholds 0.5, 0.8, 0.9.
4. uint8 outputs: the share of elements whose float64 value lies within the bound of an integer is at most LOOSE_SHARE.  The value is
   taken before the clip (tests/_value_sweep.py: near_integer): with saturated elements counted -- they are exactly 0 or 255 after it --
   the Reinhard share of set A is 0.132, over the cap; they are held to exactly 0 / 255 instead, the stricter reading.

The same four kinds of condition for the stain sweeps (tests/test_value_sweep_stains_gpu.py), on sets A, A_small, B, C and the
concentration set K: float32 evaluations of separation, jitter, deconvolution and combine within CONC_TOL / 4 and TOL_255 / 4 of
float64, the oracle's LAB round trip within 2.5e-5 of the luminosity map at L_p = 30, 75 and 100; every branch of the luminosity pass
and its clamp at 100 both ways at a gain above 1; the near-integer share of every uint8 reference under LOOSE_SHARE; and quantify's
undecided pixels (near a bin edge, or at the pole) under NEAR_EDGE_CAP.  Every figure is printed (-s); DESIGN.md 5e quotes them.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from tests import _deconv_numpy as dn
from tests import _luminosity_numpy as ln
from tests import _masked_numpy as mn
from tests import _quantify_numpy as qn
from tests import _separate_numpy as sep_np
from tests import _value_sweep as vs
from tests.test_apply_gpu import LOOSE_SHARE, TOL_255, restated
from tests.test_quantify_cpu import NEAR_EDGE_CAP

F32 = np.float32
SETS = {"A": vs.set_a, "B_bf16": lambda: vs.set_b(torch.bfloat16), "B_f16": lambda: vs.set_b(torch.float16), "C": vs.set_c}
FLOAT_SETS = ("B_bf16", "B_f16", "C")


def oracle_reinhard(x32: np.ndarray) -> np.ndarray:
    """The float32 oracle's apply with the fixed statistics on (P, 3) unit pixels, slice by slice: (P, 3) float32 in [0, 1]."""
    st = vs.statistics()
    out = np.empty_like(x32)
    for s in range(0, len(x32), vs.SLICE):
        part = np.ascontiguousarray(x32[s:s + vs.SLICE].T).reshape(1, 3, 1, -1)
        mask = np.ones((1, 1, part.shape[3]), dtype=bool)
        with np.errstate(invalid="ignore", over="ignore"):      # (the branch that is not taken: a power of a negative base, as in the float64 reference)
            out[s:s + vs.SLICE] = mn.reinhard_apply(part, st["mean"][None], st["std"][None], st["ref_mean"], st["ref_std"], mask)[0, :, 0].T
    return out


def oracle_macenko(x32: np.ndarray) -> np.ndarray:
    st = vs.statistics()
    out = np.empty_like(x32)
    for s in range(0, len(x32), vs.SLICE):
        part = np.ascontiguousarray(x32[s:s + vs.SLICE].T).reshape(1, 3, 1, -1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out[s:s + vs.SLICE] = restated(part, st["he"][None], st["max_c"][None], st["sm"], st["tmc"])[0, :, 0].T
    return out


@pytest.mark.parametrize("name", list(SETS))
def test_float32_oracle_within_a_quarter_of_the_bound_of_float64(name):
    sweep = SETS[name]()
    dom = sweep.reinhard_domain
    err = np.abs(oracle_reinhard(sweep.x32[dom]).astype(np.float64) - sweep.reinhard["out"][dom])
    print(f"{name}: Reinhard oracle against float64 on {int(dom.sum())} pixels of the domain: max {err.max():.3e} (bound {vs.REINHARD_TOL / 4:.2e})")
    assert err.max() <= vs.REINHARD_TOL / 4
    dom = sweep.macenko_domain
    err = np.abs(oracle_macenko(sweep.x32[dom]).astype(np.float64) - sweep.macenko["out"][dom])
    print(f"{name}: Macenko oracle against float64 on {int(dom.sum())} pixels in [-1/512, 2]: max {err.max():.3e} on 0-255 (bound {TOL_255 / 4:.3e})")
    assert err.max() <= TOL_255 / 4


@pytest.mark.parametrize("name", FLOAT_SETS)
def test_every_branch_is_taken_both_ways(name):
    sweep = SETS[name]()
    dom = sweep.reinhard_domain
    for function in ("gamma_in", "f", "f_inv", "gamma_out"):
        taken = sweep.reinhard[function][dom]
        for c in range(3):
            above, below = int(taken[:, c].sum()), int((~taken[:, c]).sum())
            print(f"{name}: {function}[{c}] above {above}, below {below}")
            assert min(above, below) >= vs.MIN_BRANCH_PIXELS, (name, function, c)


@pytest.mark.parametrize("name", list(SETS))
def test_the_rule_band_is_a_small_share(name):
    sweep = SETS[name]()
    for threshold in vs.THRESHOLDS:
        _, decided = sweep.rule(threshold, mn.L_BAND)
        share = float((~decided).mean())
        print(f"{name}: threshold {threshold}: share of pixels within {mn.L_BAND} of the cut {share:.2e} (cap {mn.BORDER_CAP})")
        assert share <= mn.BORDER_CAP


def test_uint8_outputs_near_an_integer_are_a_small_share():
    sweep = vs.set_a()
    for what, levels, bound in (("Reinhard", sweep.reinhard["raw"] * 255.0, vs.REINHARD_TOL * 255.0), ("Macenko", sweep.macenko["raw"], TOL_255)):
        share = float(vs.near_integer(levels, bound).mean())
        print(f"A: {what}: share of elements within {bound:.3e} of an integer {share:.4f} (cap {LOOSE_SHARE})")
        assert share <= LOOSE_SHARE


# ------------------------------------------------------------------------------------------------ the stain sweeps (tests/test_value_sweep_stains_gpu.py)
STAIN_SETS = {"A": vs.set_a, "A_small": vs.set_a_small, "B_bf16": lambda: vs.set_b(torch.bfloat16), "B_f16": lambda: vs.set_b(torch.float16), "C": vs.set_c}


def in_slices32(fn, x: np.ndarray) -> np.ndarray:
    """A float32 model on (P, 3) pixels, slice by slice."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.concatenate([fn(x[s:s + vs.SLICE]) for s in range(0, len(x), vs.SLICE)])


def oracle_separation(x32: np.ndarray, normalised: bool) -> tuple[np.ndarray, np.ndarray]:
    """The float32 oracle's separation (tests/_separate_numpy.py: so.optical_density, so.concentrations): (P, 2) and (P, 2, 3)."""
    st = vs.statistics()
    tile = vs._as_tile(x32)
    reference = (st["sm"], st["tmc"]) if normalised else None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        conc, levels = sep_np.separate(tile, np.ones((1, 1, tile.shape[3]), dtype=bool), st["he"][None], st["max_c"][None], reference)
    return np.ascontiguousarray(conc.reshape(2, -1).T), np.stack([vs._as_pixels(levels[s]) for s in range(2)], axis=1)


def model32_jitter(x32: np.ndarray, pair, own_basis: bool) -> np.ndarray:
    """C' = alpha C + beta and 240 exp(-B C') in plain float32 from the oracle's float32 concentrations: clipped levels (P, 3)."""
    st = vs.statistics()
    (alpha, beta), basis = pair, (st["he"] if own_basis else st["sm"]).astype(F32)
    c = so.concentrations(st["he"], so.optical_density(np.ascontiguousarray(x32.T)))
    if not own_basis:
        c = (c * (st["tmc"] / st["max_c"]).astype(F32)[:, None]).astype(F32)
    c = (np.asarray(alpha, dtype=F32)[:, None] * c + np.asarray(beta, dtype=F32)[:, None]).astype(F32)
    return np.clip(F32(so.IO) * np.exp(-(basis @ c)).astype(F32), 0, 255).T


def model32_deconv(x32: np.ndarray, name: str) -> dict:
    """C = inv(B) OD, C' = alpha C + beta, level = 240 exp(-B C') in plain float32: ``conc`` (P, 3) and the clipped levels."""
    basis, other = vs.basis_of(name).astype(F32), vs.basis_of(vs.OTHER_BASIS[name]).astype(F32)
    c = (np.linalg.inv(basis.astype(np.float64)).astype(F32) @ so.optical_density(np.ascontiguousarray(x32.T))).astype(F32)
    jittered = (np.asarray(dn.ALPHA, dtype=F32)[:, None] * c + np.asarray(dn.BETA, dtype=F32)[:, None]).astype(F32)
    level = lambda b, conc: np.clip(F32(so.IO) * np.exp(-(b @ conc)).astype(F32), 0, 255).T      # noqa: E731
    return {"conc": c.T, "apply": level(basis, jittered), "target": level(other, c), "stains": np.stack([level(basis[:, s:s + 1], c[s:s + 1]) for s in range(3)], axis=1)}


def quarter(what: str, err: np.ndarray, bound: float) -> None:
    worst = float(err.max(initial=0.0))
    print(f"{what}: max {worst:.3e} on {err.shape[0]} pixels (a quarter of the bound: {bound / 4:.3e})")
    assert worst <= bound / 4, (what, worst)


@pytest.mark.parametrize("name", list(STAIN_SETS))
def test_float32_restatements_of_the_stain_kernels_within_a_quarter_of_the_bound(name):
    """Condition 1 for separation, given-basis jitter and deconvolution: inside vs.Sweep.macenko_domain a float32 evaluation -- the
    oracle's functions where there are some, a plain numpy float32 model elsewhere -- is within CONC_TOL / 4 and TOL_255 / 4 of the
    float64 references, so three quarters of each bound are the kernel's."""
    sweep = STAIN_SETS[name]()
    dom = sweep.macenko_domain
    x = sweep.x32[dom]
    st = vs.statistics()
    scale = (st["tmc"].astype(np.float64) / st["max_c"].astype(np.float64))
    print(f"{name}: normalised mode scales the concentrations by {scale}; max |C| own basis {np.abs(sweep.separation['conc'][dom]).max():.2f}")
    for normalised in (False, True):
        mode = "normalised" if normalised else "own"
        conc, levels = (np.concatenate(parts) for parts in zip(*[oracle_separation(x[s:s + vs.SLICE], normalised) for s in range(0, len(x), vs.SLICE)]))
        want = sweep.separation["conc"][dom] * (scale if normalised else 1.0)
        quarter(f"{name}: separation {mode}: oracle concentrations against float64", np.abs(conc - want), vs.CONC_TOL)
        quarter(f"{name}: separation {mode}: oracle H / E levels against float64", np.abs(np.clip(levels, 0, 255) - np.clip(sweep.separation[mode][dom], 0, 255)), TOL_255)
        for k, pair in enumerate(vs.JITTER):
            got = in_slices32(lambda part: model32_jitter(part, pair, not normalised), x)
            ref = vs._in_slices(lambda part: vs.macenko64(part, st["he"], st["max_c"], st["sm"], st["tmc"], alpha=pair[0], beta=pair[1], own_basis=not normalised), x)
            quarter(f"{name}: jitter {mode} pair {k}: float32 model against float64", np.abs(got - ref["out"]), TOL_255)
    for basis in vs.DECONV_NAMES:
        ref = sweep.deconv(basis)
        got = {key: np.concatenate([model32_deconv(x[s:s + vs.SLICE], basis)[key] for s in range(0, len(x), vs.SLICE)]) for key in ("conc", "apply", "target", "stains")}
        print(f"{name}: {basis}: max |C| on the domain {np.abs(ref['conc'][dom]).max():.2f}")
        quarter(f"{name}: deconv {basis}: float32 concentrations against float64", np.abs(got["conc"] - ref["conc"][dom]), vs.CONC_TOL)
        for key in ("apply", "target", "stains"):
            quarter(f"{name}: deconv {basis} {key}: float32 levels against float64", np.abs(got[key] - np.clip(ref[key][dom], 0, 255)), TOL_255)


def test_float32_combine_within_a_quarter_of_the_bound():
    sweep = vs.concentration_set()
    dom = vs.combine_domain(sweep)
    c = sweep.pixels.numpy()[dom]
    assert dom.sum() >= 1 << 20 and (~dom).sum() >= 1 << 12 and (len(sweep.pixels) - 1 - dom.sum()) < (1 << 13)
    for basis in vs.DECONV_NAMES:
        b = vs.basis_of(basis).astype(F32)
        got = in_slices32(lambda part: np.clip(F32(so.IO) * np.exp(-(b @ part.T)).astype(F32), 0, 255).T, c)
        quarter(f"K: combine {basis}: float32 levels against float64", np.abs(got - np.clip(vs.combine64(basis)[dom], 0, 255)), TOL_255)


@pytest.mark.parametrize("name", list(STAIN_SETS))
def test_float32_luminosity_round_trip_within_a_quarter_of_the_bound(name):
    """Condition 1 for the luminosity pass, on [0, 1] at the three gains: the oracle's float32 LAB round trip with only L* changed
    (tests/_luminosity_numpy.py: lab_round_trip) against the float64 map; and the map of tests/_value_sweep.py IS ln.standardize_unit."""
    sweep = STAIN_SETS[name]()
    dom = sweep.luminosity_domain
    x = sweep.x32[dom]
    head = vs._as_tile(x[: 1 << 16])
    for row, y_p in enumerate(vs.LUMINOSITY_Y):
        want = np.clip(sweep.luminosity["raw"][dom][:, row], 0.0, 1.0)
        if y_p != 1.0:      # (the row of gain 1 is copied through by the restatement, as the kernel copies it)
            assert np.array_equal(vs._as_pixels(ln.standardize_unit(head, np.array([y_p]))), want[: 1 << 16])
        with np.errstate(invalid="ignore", over="ignore"):
            got = np.concatenate([vs._as_pixels(ln.lab_round_trip(vs._as_tile(x[s:s + vs.SLICE]), y_p, so.rgb_to_lab, so.lab_to_rgb)) for s in range(0, len(x), vs.SLICE)])
        quarter(f"{name}: luminosity L_p = {float(ln.lightness(y_p)):.1f}: oracle round trip against float64", np.abs(got - want), vs.LUMINOSITY_TOL)


@pytest.mark.parametrize("name", FLOAT_SETS)
def test_every_branch_of_the_luminosity_pass_is_taken_both_ways(name):
    """Condition 2.  The input gamma and f do not depend on the gain; f_inv, the output gamma and the clamp min(100 L* / L_p, 100) are
    counted per row, and each has to go both ways at a gain above 1 (at gain 1 the clamp takes only white, and the row is copied)."""
    sweep = STAIN_SETS[name]()
    dom, ref = sweep.luminosity_domain, sweep.luminosity

    def both(what: str, taken: np.ndarray) -> int:
        above, below = int(taken.sum()), int((~taken).sum())
        print(f"{name}: {what} above {above}, below {below}")
        return min(above, below)

    for function in ("gamma_in", "f"):
        for c in range(3):
            assert both(f"{function}[{c}]", ref[function][dom][:, c]) >= vs.MIN_BRANCH_PIXELS, (name, function, c)
    for function in ("f_inv", "gamma_out"):
        for c in range(3):
            counts = [both(f"{function}[{c}] at Y_p = {y_p:.4f}", ref[function][dom][:, row, c]) for row, y_p in enumerate(vs.LUMINOSITY_Y)]
            assert max(counts[:2]) >= vs.MIN_BRANCH_PIXELS, (name, function, c, counts)
    # (the clamp takes L* > L_p: at L_p = 75 only the few 16-bit patterns of the light quarter of the grey axis, at L_p = 30 half of a set)
    counts = [both(f"clamp at Y_p = {y_p:.4f}", ref["clamp"][dom][:, row]) for row, y_p in enumerate(vs.LUMINOSITY_Y[:2])]
    assert max(counts) >= vs.MIN_BRANCH_PIXELS, (name, counts)


def share_of(what: str, raw_levels: np.ndarray, bound: float) -> None:
    share = float(vs.near_integer(raw_levels, bound).mean())
    print(f"{what}: share of elements within {bound:.3e} of an integer {share:.4f} (cap {LOOSE_SHARE})")
    assert share <= LOOSE_SHARE, (what, share)


@pytest.mark.parametrize("name", ["A", "A_small"])
def test_uint8_outputs_of_the_stain_kernels_near_an_integer_are_a_small_share(name):
    """Condition 3, before the clip, for every uint8 reference of the stain sweeps."""
    sweep = STAIN_SETS[name]()
    for mode in ("own", "normalised"):
        for s, stain in enumerate("HE"):
            share_of(f"{name}: separation {mode} {stain} image", sweep.separation[mode][:, s], TOL_255)
    for layout in vs.stain_layouts(sweep):
        listed = np.broadcast_to((layout.index != len(sweep.pixels) - 1).reshape(layout.n, 1, layout.h, layout.w), (layout.n, 3, layout.h, layout.w))      # (not the padding)
        for own in (False, True):
            for shift in vs.row_shifts(layout, len(vs.JITTER)):
                ref = sweep.jitter(layout, own, shift)
                for k in sorted(set(ref["pair"].tolist())):
                    share_of(f"{name}: jitter {'own' if own else 'normalised'} pair {k} ({layout.name})", ref["raw"][ref["pair"] == k][listed[ref["pair"] == k]], TOL_255)
    for basis in vs.DECONV_NAMES:
        ref = sweep.deconv(basis)
        for key in ("apply", "target"):
            share_of(f"{name}: deconv {basis} {key}", ref[key], TOL_255)
        for s in range(3):
            share_of(f"{name}: deconv {basis} stain image {s}", ref["stains"][:, s], TOL_255)
    for row, y_p in enumerate(vs.LUMINOSITY_Y[:2]):      # (the row of gain 1 is a copy, compared bit for bit)
        share_of(f"{name}: luminosity Y_p = {y_p:.4f}", sweep.luminosity["raw"][:, row] * 255.0, vs.LUMINOSITY_TOL * 255.0)


def test_uint8_outputs_of_combine_near_an_integer_are_a_small_share():
    dom = vs.combine_domain(vs.concentration_set())
    for basis in vs.DECONV_NAMES:
        share_of(f"K: combine {basis}", vs.combine64(basis)[dom], TOL_255)


@pytest.mark.parametrize("name", list(STAIN_SETS))
def test_quantify_leaves_few_pixels_undecided(name):
    """Condition 4: per set and stain, the in-domain pixels within CONC_TOL of a bin edge (qn.near_edge at bin_log2 = 5) and the pixels
    with a member whose 255 x + 1 lies within POLE_BAND of zero."""
    sweep = STAIN_SETS[name]()
    k = vs.QUANTIFY_BINNING[0]
    with np.errstate(invalid="ignore"):
        at_pole = (np.abs(sweep.x32.astype(np.float64) * 255.0 + 1.0) <= vs.POLE_BAND).any(axis=1)
    for basis in vs.DECONV_NAMES:
        conc = sweep.deconv(basis)["conc"]
        for s in range(3):
            with np.errstate(invalid="ignore"):      # (outside the domain a concentration may be Inf)
                share = float((qn.near_edge(conc[:, s], k) & sweep.macenko_domain).mean() + at_pole.mean())
            print(f"{name}: {basis} stain {s}: share of pixels not decided {share:.2e} ({int(at_pole.sum())} at the pole; cap {NEAR_EDGE_CAP})")
            assert share <= NEAR_EDGE_CAP, (name, basis, s, share)


def test_the_sets_of_the_stain_sweeps_hold_what_they_say():
    small = vs.set_a_small()
    layout, = small.layouts.values()
    px = small.pixels.numpy()
    assert layout.w % 2 == 1 and (layout.h * layout.w) % 2 == 1 and layout.h * layout.w >= 2 * 16384 and layout.n >= 2
    assert all(set(px[:7 * 256, c].tolist()) == set(range(256)) for c in range(3)) and len(px) == 7 * 256 + (1 << 16) + 1
    assert sorted(np.unique(layout.index).tolist()) == list(range(len(px)))
    k = vs.concentration_set()
    for layout in k.layouts.values():
        assert set(np.unique(layout.index).tolist()) == set(range(len(k.pixels)))
    assert k.layouts["packs"].packs and not k.layouts["odd"].packs
    assert [round(float(ln.lightness(y)), 3) for y in vs.LUMINOSITY_Y] == [30.0, 75.0, 100.0] and vs.LUMINOSITY_Y[2] == 1.0
    # the rows that copy their tile through: no percentile, a black one, and Y_p = 1 exactly (gain 1) -- not its float32 neighbour
    assert ln.gain(np.array([np.nan, 0.0, 1.0, float(np.nextafter(F32(1), F32(0))), 0.5]))[1].tolist() == [True, True, True, False, False]


def test_gate_tiles_hold_what_they_say():
    """The tiles of the code-gate test (tests/test_value_sweep_gpu.py): which elements are off their grey level, by how much, and where."""
    images, tiles = vs.gate_tiles()
    n, h, w = vs.GATE_SHAPE
    x = images.numpy().reshape(n, 3, h * w)
    assert n * h * w >= 1 << 20 and (h * w) % 4 == 0 and x.min() >= 0 and x.max() <= 1
    level = np.rint(x * F32(255.0)).astype(np.int64)
    lattice = np.arange(256, dtype=F32) / F32(255.0)
    steps = x.view(np.int32).astype(np.int64) - lattice[level].view(np.int32)      # (values of [0, 1]: the bit patterns are ordered; -0.0 is far off)
    for name, t in tiles.items():
        off = steps[t] != 0
        if name.startswith("levels"):
            assert not off.any(), name
        elif name.startswith("all"):
            assert off.all() and (np.abs(steps[t]) == 1).all(), name
            assert {"all up": (steps[t] == 1) | (level[t] == 255), "all down": (steps[t] == -1) | (level[t] == 0), "all mixed": np.abs(steps[t].mean()) < 0.01}[name].all(), name
        else:
            spot, kind = name.rsplit(" ", 1)
            c, p = vs.GATE_SPOTS[spot]
            assert off.sum() == 1 and off[c, p], name
            if kind == "-0":
                assert np.signbit(x[t, c, p]) and x[t, c, p] == 0 and np.signbit(x[t]).sum() == 1, name
            else:
                assert steps[t, c, p] == {"up": 1, "down": -1}[kind] and level[t, c, p] == vs.GATE_MOVED_PIXEL[c], name
    packs = h * w // 4
    assert [p // 4 for _, p in vs.GATE_SPOTS.values()] == [0, packs // 2 + 29, packs - 1] and (packs // 2 + 29) % 64 == 29


def test_gate_and_half_ulp_helpers():
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, np.nextafter(F32(1), F32(0)), 0.5, 3.4e38, -1.0, 254.5 / 255], dtype=F32)
    assert vs.grey_levels(x).tolist() == [0, 255, 0, 0, 255, 254, 127, 255, 0, 254]
    ref = np.array([0.3, 1.0, 200.0, 3e-6, 0.0])
    assert vs.half_ulp(ref, torch.bfloat16).tolist() == [2.0 ** -10, 2.0 ** -8, 0.5, 2.0 ** -27, 2.0 ** -134]
    assert vs.half_ulp(ref, torch.float16).tolist() == [2.0 ** -13, 2.0 ** -11, 2.0 ** -4, 2.0 ** -25, 2.0 ** -25]
