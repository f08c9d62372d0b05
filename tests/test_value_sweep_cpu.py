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
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _masked_numpy as mn
from tests import _value_sweep as vs
from tests.test_apply_gpu import LOOSE_SHARE, TOL_255, restated

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
