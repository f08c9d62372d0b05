"""What tests/test_param_sweep_gpu.py relies on, measured without a GPU: the verified PARAMETER domain of every family of
tests/_param_sweep.py.  For each row the project's float32 model of the operation -- ``fold_restated`` (tests/test_apply_gpu.py), the
oracle's functions (``so.*`` through tests/_separate_numpy.py and tests/_masked_numpy.py), plain float32 numpy for the jitter and the
three-stain calls, the oracle's LAB round trip (tests/_luminosity_numpy.py) -- is compared with the float64 reference over the pixel
lists of all four element types.  The margin is measured against float64, never against a kernel.

* A row INSIDE its domain (the constants of tests/_param_sweep.py) keeps the model within a quarter of the project's unchanged bound
  (TOL_255 2.55e-2 on levels, CONC_TOL 3e-5 on concentrations, REINHARD_TOL and LUMINOSITY_TOL 1e-4 on [0, 1]): three quarters are the
  kernel's.  Rows outside are printed, not held: the domains are narrowed to simple functions of a row, so some rows outside would pass.
* Every estimated row is inside; each family keeps at least five constructed rows inside and five outside.
* The share of a uint8 reference within the bound of an integer stays under LOOSE_SHARE (12 %) for every row inside.

Run with ``-s`` for the figures (DESIGN.md 5e quotes them)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import stain_oracle as so
from tests import _deconv_numpy as dn
from tests import _hm_slide_numpy as sn
from tests import _luminosity_numpy as ln
from tests import _masked_numpy as mn
from tests import _param_sweep as ps
from tests import _separate_numpy as sep_np
from tests import _value_sweep as vs
from tests.test_apply_gpu import LOOSE_SHARE, TOL_255, fold_restated

F32, F64 = np.float32, np.float64
KINDS = tuple(ps.DTYPES)
MIN_ROWS = 5


def worst_per_row(model: np.ndarray, raw: np.ndarray, top: float | None) -> np.ndarray:
    """(R,) the largest |model - clip(reference)| of a row; a NaN on either side counts as infinite."""
    ref = raw if top is None else np.clip(raw, 0.0, top)
    with np.errstate(all="ignore"):
        err = np.abs(model.astype(F64) - ref)
    return np.where(np.isnan(err), np.inf, err).reshape(len(err), -1).max(axis=1)


def near_share(raw_levels: np.ndarray, bound: float) -> np.ndarray:
    """(R,) the share of a row's uint8 reference within ``bound`` of an integer (vs.near_integer: before the clip, saturated ones not counted)."""
    return vs.near_integer(raw_levels, bound).reshape(len(raw_levels), -1).mean(axis=1)


def hold(rows: ps.Rows, what: str, err: np.ndarray, bound: float, share: np.ndarray | None = None, counts: bool = True) -> None:
    quarter = bound / 4
    print(f"\n{rows.family}: {what}: float32 model against float64, worst over {', '.join(KINDS)}; a quarter of the bound is {quarter:.3e}")
    for i, name in enumerate(rows.names):
        tail = "" if share is None else f"   near-integer share of the uint8 reference {share[i]:.3f}"
        print(f"  {'estimated  ' if rows.estimated[i] else 'constructed'} {'inside ' if rows.inside[i] else 'OUTSIDE'} {name:<34} {err[i]:.3e}{'' if err[i] <= quarter else '  > quarter'}{tail}")
    inside = rows.inside
    print(f"  inside: worst {err[inside].max():.3e}; {int((inside & ~rows.estimated).sum())} constructed rows inside, {int((~inside & ~rows.estimated).sum())} outside, "
          f"{int((~inside & (err <= quarter)).sum())} rows outside that the model would pass")
    assert (err[inside] <= quarter).all(), (what, [rows.names[i] for i in np.flatnonzero(inside & (err > quarter))])
    assert inside[rows.estimated].all(), (what, "an estimated row is outside the domain", [rows.names[i] for i in np.flatnonzero(rows.estimated & ~inside)])
    if counts:
        assert (inside & ~rows.estimated).sum() >= MIN_ROWS and (~inside & ~rows.estimated).sum() >= MIN_ROWS, what
    if share is not None:
        assert (share[inside] <= LOOSE_SHARE).all(), (what, [(rows.names[i], float(share[i])) for i in np.flatnonzero(inside & (share > LOOSE_SHARE))])


def levels_of(kind: str) -> np.ndarray:
    """(3, P) float32 grey levels 0..255 of the pixel list, as the fold reads them (uint8: the byte; floats: 255 x in float32)."""
    return np.ascontiguousarray((ps.x32(kind) * F32(255.0)).astype(F32).T) if kind != "u8" else np.ascontiguousarray(ps.pixels("u8").numpy().astype(F32).T)


# ------------------------------------------------------------------------------------------------ H&E sources
@pytest.mark.parametrize("reference", list(ps.he_references()))
def test_he_sources_domain(reference):
    """Candidate 1 of the issue: the fold's float32 model against float64 as E moves towards H."""
    rows = ps.he_sources()
    sm, tmc = ps.he_references()[reference]
    err = np.zeros(len(rows))
    for kind in KINDS:
        lv = levels_of(kind)
        model = np.stack([fold_restated(lv, rows.params["he"][i], rows.params["max_c"][i], sm, tmc).T for i in range(len(rows))])
        err = np.maximum(err, worst_per_row(model, ps.he_sources64(kind, reference), 255.0))
    print("\n  " + "; ".join(f"{n}: angle {ps.he_angle(h):.4f} rad, cond {ps.he_cond(h):.1f}" for n, h in zip(rows.names, rows.params["he"]) if n.startswith("E moved")))
    print(f"  estimated rows: cond(HE) {min(ps.he_cond(h) for h in rows.params['he'][rows.estimated]):.1f} ... {max(ps.he_cond(h) for h in rows.params['he'][rows.estimated]):.1f}, "
          f"scale {np.min(tmc / rows.params['max_c'][rows.estimated]):.2f} ... {np.max(tmc / rows.params['max_c'][rows.estimated]):.2f}")
    hold(rows, f"apply, reference {reference}", err, TOL_255, near_share(ps.he_sources64("u8", reference), TOL_255))


@pytest.mark.parametrize("reference", list(ps.he_references()))
def test_he_separation_domain(reference):
    """The oracle's float32 separation with a given basis: H / E levels against TOL_255 on the domain of the apply.  The bound on the
    CONCENTRATIONS is absolute, so it is a bound on their size too: they are held where also the gain max(scale) / sigma_min(HE) of the
    map from optical density to concentration stays under HE_CONC_GAIN_CAP."""
    rows = ps.he_sources()
    ref_pair = ps.he_references()[reference]
    tile_of = {kind: vs._as_tile(ps.x32(kind)) for kind in KINDS}
    ones = np.ones((1, 1, ps.N_PIXELS + 1), dtype=bool)
    for mode in ("own", "normalised"):
        err_levels, err_conc, size = np.zeros(len(rows)), np.zeros(len(rows)), np.zeros(len(rows))
        for kind in KINDS:
            ref = ps.he_separation64(kind, reference)
            conc, levels = [], []
            with np.errstate(all="ignore"):
                for i in range(len(rows)):
                    c, lv = sep_np.separate(tile_of[kind], ones, rows.params["he"][i][None], rows.params["max_c"][i][None], ref_pair if mode == "normalised" else None)
                    conc.append(c.reshape(2, -1).T)
                    levels.append(np.stack([vs._as_pixels(lv[s]) for s in range(2)]))
                want = ref["conc"] * (ref["scale"][:, None, :] if mode == "normalised" else 1.0)
                size = np.maximum(size, np.where(np.isfinite(want), np.abs(want), np.inf).reshape(len(rows), -1).max(axis=1))
            err_conc = np.maximum(err_conc, worst_per_row(np.stack(conc), want, None))
            err_levels = np.maximum(err_levels, worst_per_row(np.clip(np.stack(levels), 0, 255), ref[mode], 255.0))
        u8 = ps.he_separation64("u8", reference)[mode]
        hold(rows, f"separation {mode} H / E levels, reference {reference}", err_levels, TOL_255, near_share(u8, TOL_255))
        with np.errstate(all="ignore"):
            gain = np.array([ps.he_conc_gain(rows.params["he"][i], ps.he_scales(rows.params["he"][i], rows.params["max_c"][i], ref_pair[1]) * np.linalg.norm(rows.params["he"][i].astype(F64), axis=0)
                                             if mode == "normalised" else None) for i in range(len(rows))])
        held = rows.inside & (gain <= ps.HE_CONC_GAIN_CAP)
        print(f"\n  {mode} concentrations, reference {reference} (a quarter of CONC_TOL: {vs.CONC_TOL / 4:.2e}; held: inside and gain <= {ps.HE_CONC_GAIN_CAP})")
        for i, n in enumerate(rows.names):
            print(f"  {'held    ' if held[i] else 'not held'} {n:<34} gain {gain[i]:9.3g}  |C| <= {size[i]:9.3g}  err {err_conc[i]:.3e}{'' if err_conc[i] <= vs.CONC_TOL / 4 else '  > quarter'}")
        assert (err_conc[held] <= vs.CONC_TOL / 4).all(), [rows.names[i] for i in np.flatnonzero(held & (err_conc > vs.CONC_TOL / 4))]
        assert held[rows.estimated].all(), [rows.names[i] for i in np.flatnonzero(rows.estimated & ~held)]


def model32_jitter(x: np.ndarray, alpha, beta, own_basis: bool) -> np.ndarray:
    """tests/test_value_sweep_cpu.py's model: C' = alpha C + beta and 240 exp(-B C') in plain float32 from the oracle's concentrations."""
    st = vs.statistics()
    basis = (st["he"] if own_basis else st["sm"]).astype(F32)
    with np.errstate(all="ignore"):
        c = so.concentrations(st["he"], so.optical_density(np.ascontiguousarray(x.T)))
        if not own_basis:
            c = (c * (st["tmc"] / st["max_c"]).astype(F32)[:, None]).astype(F32)
        c = (np.asarray(alpha, dtype=F32)[:, None] * c + np.asarray(beta, dtype=F32)[:, None]).astype(F32)
        out = np.clip(F32(so.IO) * np.exp(-(basis @ c)).astype(F32), 0, 255).T
    return out


@pytest.mark.parametrize("own_basis", [False, True], ids=["normalised", "own"])
def test_he_factors_domain(own_basis):
    rows = ps.he_factors()
    err = np.zeros(len(rows))
    for kind in KINDS:
        model = np.stack([model32_jitter(ps.x32(kind), rows.params["alpha"][i], rows.params["beta"][i], own_basis) for i in range(len(rows))])
        err = np.maximum(err, worst_per_row(model, ps.he_factors64(kind, own_basis), 255.0))
    hold(rows, f"jitter, {'own basis' if own_basis else 'normalised'}", err, TOL_255, near_share(ps.he_factors64("u8", own_basis), TOL_255))


# ------------------------------------------------------------------------------------------------ three-stain bases
def model32_deconv(x: np.ndarray, basis: np.ndarray, target: np.ndarray, combine_input: np.ndarray) -> dict:
    """tests/test_value_sweep_cpu.py's model per row: C = inv(B) OD, C' = alpha C + beta, level = 240 exp(-B C') in plain float32."""
    with np.errstate(all="ignore"):
        c = (np.linalg.inv(basis.astype(F64)).astype(F32) @ so.optical_density(np.ascontiguousarray(x.T))).astype(F32)
        jittered = (np.asarray(dn.ALPHA, dtype=F32)[:, None] * c + np.asarray(dn.BETA, dtype=F32)[:, None]).astype(F32)
        level = lambda b, conc: np.clip(F32(so.IO) * np.exp(-(b @ conc)).astype(F32), 0, 255).T      # noqa: E731
        return {"conc": c.T, "apply": level(basis, jittered), "target": level(target, c), "stains": np.stack([level(basis[:, s:s + 1], c[s:s + 1]) for s in range(3)]),
                "combine": level(basis, combine_input.reshape(3, -1))}


def test_bases_domain():
    rows = ps.bases()
    ok = ps.basis_defined(rows)
    err = {key: np.zeros(len(rows)) for key in ("conc", "apply", "target", "stains", "combine")}
    for kind in KINDS:
        ref = ps.bases64(kind)
        models = [model32_deconv(ps.x32(kind), rows.params["basis"][i], rows.params["target"][i], ps.combine_input(kind)) if ok[i] else None for i in range(len(rows))]
        for key in err:
            model = np.stack([m[key] if m is not None else np.full(ref[key].shape[1:], np.nan) for m in models])
            err[key] = np.maximum(err[key], worst_per_row(model, ref[key], None if key == "conc" else 255.0))
    with np.errstate(all="ignore"):
        print("\n  |det|: " + "; ".join(f"{n}: {abs(np.linalg.det(b.astype(F64))):.3g}" for n, b in zip(rows.names, rows.params["basis"])))
    u8 = ps.bases64("u8")
    hold(rows, "concentrations", err["conc"], vs.CONC_TOL)
    for key in ("apply", "target", "combine"):
        hold(rows, f"{key} levels", err[key], TOL_255, near_share(u8[key], TOL_255))
    hold(rows, "stain images", err["stains"], TOL_255, near_share(u8["stains"], TOL_255))


# ------------------------------------------------------------------------------------------------ Reinhard statistics
@pytest.mark.parametrize("reference", list(ps.reinhard_references()))
def test_reinhard_domain(reference):
    rows = ps.reinhard()
    rm, rs = ps.reinhard_references()[reference]
    err = np.zeros(len(rows))
    ones = np.ones((1, 1, ps.N_PIXELS + 1), dtype=bool)
    for kind in KINDS:
        tile = vs._as_tile(ps.x32(kind))
        with np.errstate(all="ignore"):
            model = np.stack([vs._as_pixels(mn.reinhard_apply(tile, rows.params["mean"][i][None], rows.params["std"][i][None], rm, rs, ones)) for i in range(len(rows))])
        nan_row = np.isnan(rows.params["mean"]).any(axis=1) | np.isnan(rows.params["std"]).any(axis=1)      # (mn.reinhard_apply copies those: the masked rule)
        e = worst_per_row(model, ps.reinhard64(kind, reference), 1.0)
        err = np.maximum(err, np.where(nan_row, np.inf, e))
    with np.errstate(all="ignore"):
        print("\n  gain ref_std / src_std: " + "; ".join(f"{n}: {float((rs.astype(F64) / s.astype(F64)).max()):.3g}" for n, s in zip(rows.names, rows.params["std"])))
    hold(rows, f"apply, reference {reference}", err, vs.REINHARD_TOL, near_share(ps.reinhard64("u8", reference) * 255.0, vs.REINHARD_TOL * 255.0))


# ------------------------------------------------------------------------------------------------ lookup tables
def test_tables_domain_and_rule():
    """The lookup is exact arithmetic, so there is no margin to measure: the domain is where the reference's own cast is defined (every
    entry finite and inside 0..255); outside it the library's rule holds (clamp before the cast of every output type, a NaN entry is 0:
    candidate 2 of the issue).  Inside, sn.lookup is the reference's arithmetic unchanged: the rule changes no bit there."""
    rows = ps.tables()
    assert rows.inside[rows.estimated].all()
    assert (rows.inside & ~rows.estimated).sum() >= MIN_ROWS and (~rows.inside & ~rows.estimated).sum() >= MIN_ROWS
    luts = rows.params["lut"]
    for kind in KINDS:
        src = ps.images(kind, "odd", min(len(rows), ps.MAX_ROWS))
        x = src.numpy() if kind in ("u8", "f32") else src.float().numpy()
        n = len(x)
        got = sn.lookup(x, luts[:n])
        u8, scaled = so.images_to_uint8(x)
        for i in range(n):
            with np.errstate(all="ignore"):
                picked = np.stack([luts[i, c][u8[i, c]] for c in range(3)])
                if rows.inside[i]:      # the reference's own line (so.hm_transform): clip, scale, cast
                    want = so.restore_dtype(np.clip(picked / F32(255.0), F32(0), F32(1)), x.dtype, in_0_255=False) if scaled else so.restore_dtype(np.clip(picked, F32(0), F32(255)), x.dtype, in_0_255=True)
                    assert np.array_equal(got[i], want), (kind, rows.names[i])
                rule = np.clip(np.where(np.isnan(picked), F32(0), picked), F32(0), F32(255))
                want = np.clip(rule / F32(255.0), F32(0), F32(1)) if scaled else np.trunc(rule).astype(np.uint8)
                assert np.array_equal(got[i], want), (kind, rows.names[i])
                assert np.isfinite(got[i].astype(F64)).all()
    print(f"\ntables: {int(rows.inside.sum())} rows inside 0..255 ({int((rows.inside & ~rows.estimated).sum())} constructed), {int((~rows.inside).sum())} outside: "
          + ", ".join(n for n, i in zip(rows.names, rows.inside) if not i))


# ------------------------------------------------------------------------------------------------ luminosity rows
def model32_lift(tile: np.ndarray, y_p: float) -> np.ndarray:
    """The one step of the map that the oracle's round trip does not share with the kernel: f_y' = min(fma(g, f_y, s), 1) with g = 100 / L_p
    and s = (16/116)(1 - g) rounded to float32 and f_y a float32 -- the cancellation of two terms of size g / 7 on a dark pixel.  Everything
    else in float64 (tests/_luminosity_numpy.py), so the figure is the cost of that step alone.  (P, 3) unit values before the clamp."""
    g64 = ln.gain(np.array([y_p]))[0][0]
    g, s = F64(F32(g64)), F64(F32((16.0 / 116.0) * (1.0 - g64)))
    f = ln.f_values(tile)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    fy32 = fy.astype(F32).astype(F64)
    fy2 = np.minimum((g * fy32 + s).astype(F32).astype(F64), 1.0)      # (the product and the sum of float32 values in float64, rounded once: an fma)
    lin = np.einsum("ij,njhw->nihw", ln.XYZ2RGB, ln.f_inv(np.stack([fy2 + (fx - fy), fy2, fy2 - (fy - fz)], axis=1)) * ln.WHITE)
    curve = lin > 0.0031308
    return vs._as_pixels(np.where(curve, 1.055 * vs._pow(curve, lin, 1.0 / 2.4) - 0.055, 12.92 * lin))


def test_luminosity_domain():
    """Candidate 3 of the issue: the oracle's float32 LAB round trip with only L* changed against the float64 map, as L_p falls."""
    rows = ps.luminosity()
    copied = ps.luminosity_copied(rows)
    err, err_fold = np.zeros(len(rows)), np.zeros(len(rows))
    with np.errstate(all="ignore"):
        l_p = ln.lightness(rows.params["y"].astype(F64))
        gain32 = (100.0 / l_p).astype(F32)
    for kind in KINDS:
        x = ps.x32(kind)
        tile = vs._as_tile(x)
        model = []
        with np.errstate(all="ignore"):
            for i in range(len(rows)):
                model.append(x.astype(F64) if copied[i] else vs._as_pixels(ln.lab_round_trip(tile, float(rows.params["y"][i]), so.rgb_to_lab, so.lab_to_rgb)))
            fold = np.stack([x.astype(F64) if copied[i] else model32_lift(tile, float(rows.params["y"][i])) for i in range(len(rows))])
        ref = ps.luminosity64(kind)
        err = np.maximum(err, worst_per_row(np.stack(model), ref, 1.0))
        err_fold = np.maximum(err_fold, worst_per_row(np.clip(fold, 0.0, 1.0), ref, 1.0))
    print("\n  " + "; ".join(f"{n}: Y_p {y:.4g}, L_p {l:.4g}, float32 gain {g:.4g}{' (copied)' if c else ''}" for n, y, l, g, c in zip(rows.names, rows.params["y"], l_p, gain32, copied)))
    share = np.where(copied, 0.0, near_share(ps.luminosity64("u8") * 255.0, vs.LUMINOSITY_TOL * 255.0))      # (a copied row is compared bit for bit)
    hold(rows, "apply, the oracle's LAB round trip", err, vs.LUMINOSITY_TOL, share)
    hold(rows, "apply, float32 lift g f_y + (16/116)(1 - g)", err_fold, vs.LUMINOSITY_TOL)
    # Candidate 3 of the issue, first half: "for a positive Y_p below about 3e-40 the float32 gain is +Inf".  It is not reached: L_p =
    # 116 (7.787 Y_p + 16/116) - 16 is formed in fp64, where 7.787 Y_p below half an ulp of 16/116 (Y_p < 1.8e-18) is absorbed and L_p is
    # exactly 0 -- a black row, copied.  The smallest positive L_p is a few ulps of 16 (3.6e-15), its gain (2.8e16) a finite float32.
    assert copied[rows.index("denormal")] and copied[rows.index("smallest normal")] and copied[rows.index("1")] and copied[rows.index("NaN")] and copied[rows.index("-0.0")]
    y = np.concatenate([np.logspace(-45, -10, 20001).astype(F32), vs._neighbours(np.array([1.8e-18, 1e-17, 1e-16], dtype=F32), 2000)])
    y = y[y > 0]
    with np.errstate(all="ignore"):
        lp = ln.lightness(y.astype(F64))
        g32 = (100.0 / lp[lp > 0]).astype(F32)
    print(f"\n  positive float32 Y_p from {y.min():.3g}: L_p is exactly 0 up to Y_p = {y[lp <= 0].max():.4g}, the smallest positive L_p is {lp[lp > 0].min():.3g}, the largest float32 gain {g32.max():.4g}")
    assert (lp >= 0).all() and np.isfinite(g32).all() and y[lp <= 0].max() < 1e-17 and not ln.gain(y[lp <= 0])[1].__invert__().any()
    black = ps.luminosity64("u8")[:, 0]      # (pixel 0 of the list is the grey axis at level 0)
    assert (ps.pixels("u8")[0] == 0).all() and np.abs(black[~copied & np.isfinite(rows.params["y"])]).max() <= 1e-9, "the float64 map keeps black black at every gain"
