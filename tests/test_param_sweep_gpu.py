"""Every PARAMETER family of tests/_param_sweep.py through the entry points that take their statistics as arguments, against float64
(what the domains rely on: tests/test_param_sweep_cpu.py; the sibling of the value sweeps, whose helpers it imports).  One tile per
row, uint8 / float32 / bf16 / f16, a pack layout and an odd one, aligned and one element off a 16-byte address, channels-last where the
entry point has the form.

1. Rows INSIDE the domain: check_tiles' and check_concentrations' rules against float64 -- the project's bound, plus half an ulp for
   16-bit outputs, uint8 equal to the truncated float64 value except within the bound of an integer.
2. EVERY row, inside or not: every image element is finite and inside the output range (a singular three-stain basis is undefined by
   the header: only isolation is held there).
3. Indexing and isolation: tile t of the n_sources = N call has the bits of an n_sources = 1 call on that tile with row t; replacing
   rows by other rows changes no bit of any other tile; the masked call with all ones has the unmasked call's bits row by row, and a
   tile whose row holds a NaN follows the header's copy / background rule.
4. Rules the header states exactly: a zero maxC saturates as the fold does, a rank-1 HE gives E = 0, the identity factors give the bits
   of the call without factors, luminosity rows that are NaN, have L_p <= 0 or equal 1 are copied, the identity table on uint8 is a copy,
   a table entry outside 0..255 is clamped before the cast of every type and a NaN entry is 0.

Measured with two loosened kernels in a scratch build: the source row of sx_macenko_apply read as ``tile % 2``, and the
fold matrix M rounded to bf16 -- each fails this file."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import ColorDeconvolution, HistogramMatching, LuminosityStandardizer, Macenko, Reinhard, synth
from tests import _deconv_numpy as dn
from tests import _param_sweep as ps
from tests import _quantify_numpy as qn
from tests import _value_sweep as vs
from tests.test_apply_gpu import TOL_255, fold_restated
from tests.test_hm_slide_gpu import bits, same_bits, unaligned_copy
from tests.test_macenko_mask_gpu import background_expected
from tests.test_separate_apply_gpu import no_stain_level
from tests.test_value_sweep_stains_gpu import check_concentrations, check_tiles, nchw

pytestmark = pytest.mark.gpu

KINDS = list(ps.DTYPES)
LAYOUTS = list(ps.LAYOUTS)
WORST: dict = {}      # (family, kind) -> the worst error of a float output, printed by the last test


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def on(dev, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def in_range(what, out: torch.Tensor, top: float, rows: torch.Tensor | None = None) -> None:
    """Check 2: every element finite and inside [0, top] (uint8 cannot be otherwise)."""
    if out.dtype == torch.uint8:
        return
    got = (out if rows is None else out[rows.to(out.device)]).float()
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= top, (what, "an element is not finite or outside the output range")


def note(family: str, kind: str, worst: float) -> None:
    if kind != "u8":
        WORST[(family, kind)] = max(WORST.get((family, kind), 0.0), worst)


def hold_rows(dev, what, family, kind, layout, rows: ps.Rows, call, raws: list, *, top: float, bound: float, held=None, defined=None, masked=None, nan_rule=None, nan_keys=None) -> list:
    """The four checks for one family, element type and layout.  ``call(x, idx, mask=None) -> [outputs]`` runs tiles ``x`` with the rows
    ``idx`` (as many as tiles); ``raws``: per output the float64 reference (R, P, 3) of an image on 0..top, or ("conc", (R, P, K)) for
    concentrations; ``held`` (R,): the rows checked against float64 (default rows.inside); ``defined`` (R,): the rows whose values are
    defined at all (default all); ``masked``: True where the entry point has a masked form; ``nan_rule(x_cpu, output index) -> expected
    tile`` for rows that hold a NaN in one of ``nan_keys`` (default: any parameter).  Returns the outputs of the whole call."""
    n = len(rows)
    assert n <= ps.MAX_ROWS
    idx = np.arange(n)
    held = rows.inside if held is None else held
    defined = np.ones(n, dtype=bool) if defined is None else defined
    x_cpu = ps.images(kind, layout, n)
    x = x_cpu.to(dev)
    outs = call(x, idx)
    held_t, defined_t = torch.from_numpy(held), torch.from_numpy(defined)
    everywhere = np.ones((int(held.sum()),) + ps.LAYOUTS[layout], dtype=bool)
    for k, (out, raw) in enumerate(zip(outs, raws)):
        label = f"{what} {kind} {layout} output {k}"
        if isinstance(raw, tuple):      # concentrations
            ref = ps.spread(raw[1], layout)[held]
            worst = check_concentrations(label, out[held_t.to(dev)], ref, everywhere)
            WORST[(family + " C", kind)] = max(WORST.get((family + " C", kind), 0.0), worst)
            continue
        assert out.dtype == ps.DTYPES[kind] and out.shape[0] == n, label
        note(family, kind, check_tiles(label, out[held_t.to(dev)], ps.spread(raw, layout)[held], everywhere, bound, top=top, range_everywhere=False))      # 1
        in_range(label, out, top, defined_t)                                                                                                          # 2
    # 3a: one tile, one row
    for t in range(n):
        alone = call(x[t:t + 1].clone(), idx[t:t + 1])
        for k, (a, b) in enumerate(zip(alone, outs)):
            assert same_bits(a[0], b[t]), (what, kind, layout, rows.names[t], k, "tile t of the N-row call is not the one-row call on that tile")
    # 3b: the rows outside the domain replaced by the first row inside; then one row inside replaced by its neighbour
    first = int(np.flatnonzero(held)[0])
    swapped = np.where(held, idx, first)
    again = call(x, swapped)
    for a, b in zip(again, outs):
        assert same_bits(a[held_t.to(dev)], b[held_t.to(dev)]), (what, kind, layout, "replacing the rows outside the domain changed a tile inside")
    j = int(np.flatnonzero(held)[1])
    one = idx.copy()
    one[j] = first
    keep = torch.from_numpy(idx != j).to(dev)
    again = call(x, one)
    moved = call(x[j:j + 1].clone(), np.array([first]))
    for a, b, c in zip(again, outs, moved):
        assert same_bits(a[keep], b[keep]) and same_bits(a[j], c[0]), (what, kind, layout, "replacing one row changed another tile, or tile j did not take the new row")
    # unaligned: the same bits
    for a, b in zip(call(unaligned_copy(x), idx), outs):
        assert same_bits(a, b), (what, kind, layout, "one element off a 16-byte address: other bits")
    # 3c / 3d: the masked call with all ones
    if masked:
        has_nan = np.array([any(np.isnan(rows.params[key][i]).any() for key in (nan_keys or rows.params)) for i in range(n)])
        ones = torch.ones((n,) + ps.LAYOUTS[layout], dtype=torch.uint8, device=dev)
        plain = torch.from_numpy(~has_nan).to(dev)
        for k, (a, b) in enumerate(zip(call(x, idx, mask=ones), outs)):
            assert same_bits(a[plain], b[plain]), (what, kind, layout, k, "the masked call with all ones is not the unmasked call")
            for t in np.flatnonzero(has_nan):
                want = nan_rule(x_cpu[t:t + 1], k)
                assert same_bits(a[t:t + 1].cpu(), want), (what, kind, layout, rows.names[t], k, "a masked tile whose row holds a NaN does not follow the header's rule")
    return outs


# ------------------------------------------------------------------------------------------------ H&E sources: sx_macenko_apply(_masked)
def macenko_with(dev, reference: str) -> Macenko:
    sm, tmc = ps.he_references()[reference]
    norm = Macenko(device=dev, backend="torch_hip")
    norm._stain_matrix, norm._target_max_conc = on(dev, sm), on(dev, tmc)
    norm._is_fitted = True
    return norm


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("reference", list(ps.he_references()))
def test_he_sources_apply(dev, reference, kind, layout):
    rows = ps.he_sources()
    norm = macenko_with(dev, reference)
    he, mc = on(dev, rows.params["he"]), on(dev, rows.params["max_c"])

    def call(x, idx, mask=None):
        return [norm.apply(x, (he[idx], mc[idx]), mask=mask)]

    (out,) = hold_rows(dev, f"apply, reference {reference}", "H&E apply", kind, layout, rows, call, [ps.he_sources64(kind, reference)], top=255.0, bound=TOL_255,
                       masked=True, nan_rule=lambda x_cpu, k: background_expected(x_cpu, False))
    # 4: a zero maxC saturates exactly as the fold does; a rank-1 HE drops its second singular value (the float64 lstsq reference)
    sm, tmc = ps.he_references()[reference]
    t = rows.index("maxC 0")
    levels = ps.images(kind, layout, len(rows))[t].float().reshape(3, -1).numpy()
    want = fold_restated(levels if kind == "u8" else (levels * np.float32(255.0)).astype(np.float32), rows.params["he"][t], rows.params["max_c"][t], sm, tmc)
    assert np.isin(want, (0.0, 255.0)).all() and np.array_equal(out[t].reshape(3, -1).float().cpu().numpy(), want), (kind, layout, "a zero maxC does not saturate as the fold does")
    t = rows.index("rank-1 HE")
    raw = ps.spread(ps.he_sources64(kind, reference), layout)[t:t + 1]
    check_tiles(f"apply rank-1 HE {kind} {layout}", out[t:t + 1], raw, np.ones((1,) + ps.LAYOUTS[layout], dtype=bool), TOL_255)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("own_basis", [True, False], ids=["own", "normalised"])
def test_he_sources_separation(dev, own_basis, kind, layout):
    """sx_macenko_separate_apply(_masked): concentrations where also the concentration gain is inside (tests/test_param_sweep_cpu.py)."""
    rows = ps.he_sources()
    reference = "real"
    norm = macenko_with(dev, reference)
    he, mc = on(dev, rows.params["he"]), on(dev, rows.params["max_c"])
    ref = ps.he_separation64(kind, reference)
    mode = "own" if own_basis else "normalised"
    tmc = ps.he_references()[reference][1]
    with np.errstate(all="ignore"):
        gain = np.array([ps.he_conc_gain(h, None if own_basis else ps.he_scales(h, m, tmc) * np.linalg.norm(h.astype(np.float64), axis=0)) for h, m in zip(rows.params["he"], rows.params["max_c"])])
        conc = ref["conc"] * (1.0 if own_basis else ref["scale"][:, None, :])
    held_c = rows.inside & (gain <= ps.HE_CONC_GAIN_CAP)

    def call(x, idx, mask=None):
        got = norm.separate(x, source=(he[idx], mc[idx]), own_basis=own_basis, stains=True, concentrations=True, mask=mask)
        return [got.hematoxylin, got.eosin, got.concentrations]

    level = no_stain_level(ps.DTYPES[kind], False)

    def nan_rule(x_cpu, k):
        shape = tuple(x_cpu.shape)
        return torch.zeros((1, 2) + shape[2:], dtype=torch.float32) if k == 2 else level.reshape(1, 1, 1, 1).expand(shape).contiguous()

    # (the concentrations are held on their own rows below: hold_rows takes one set of held rows)
    outs = hold_rows(dev, f"separation {mode}", f"H&E separation {mode}", kind, layout, rows, lambda x, idx, mask=None: call(x, idx, mask)[:2],
                     [np.ascontiguousarray(ref[mode][:, 0]), np.ascontiguousarray(ref[mode][:, 1])], top=255.0, bound=TOL_255)
    x = ps.images(kind, layout, len(rows)).to(dev)
    h_img, e_img, c = call(x, np.arange(len(rows)))
    assert same_bits(h_img, outs[0]) and same_bits(e_img, outs[1])
    sel = torch.from_numpy(held_c).to(dev)
    worst = check_concentrations(f"separation {mode} {kind} {layout}", c[sel], ps.spread(conc, layout)[held_c], np.ones((int(held_c.sum()),) + ps.LAYOUTS[layout], dtype=bool))
    WORST[(f"H&E separation {mode} C", kind)] = max(WORST.get((f"H&E separation {mode} C", kind), 0.0), worst)
    # 3a for the concentrations, 3c / 3d for all three outputs
    for t in (0, len(rows) // 2, len(rows) - 1):
        assert same_bits(call(x[t:t + 1].clone(), np.array([t]))[2][0], c[t])
    n = len(rows)
    has_nan = np.isnan(rows.params["he"]).any(axis=(1, 2)) | (np.isnan(rows.params["max_c"]).any(axis=1) & (not own_basis))      # (maxC is not read in the own basis)
    ones = torch.ones((n,) + ps.LAYOUTS[layout], dtype=torch.uint8, device=dev)
    plain = torch.from_numpy(~has_nan).to(dev)
    for k, (a, b) in enumerate(zip(call(x, np.arange(n), mask=ones), (h_img, e_img, c))):
        assert same_bits(a[plain], b[plain]), (mode, kind, layout, k, "the masked separation with all ones is not the unmasked one")
        for t in np.flatnonzero(has_nan):
            assert same_bits(a[t:t + 1].cpu(), nan_rule(ps.images(kind, layout, n)[t:t + 1], k)), (mode, kind, layout, rows.names[t], k)
    # 4: a rank-1 HE gives E = 0, exactly
    t = rows.index("rank-1 HE")
    assert not bool((c[t, 1] != 0).any()), (mode, kind, layout, "a rank-1 HE does not give E = 0")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("own_basis", [False, True], ids=["normalised", "own"])
def test_he_factors(dev, own_basis, kind, layout):
    rows = ps.he_factors()
    norm = macenko_with(dev, "real")
    st = vs.statistics()
    source = (on(dev, st["he"]).reshape(1, 3, 2), on(dev, st["max_c"]).reshape(1, 2))
    alpha, beta = on(dev, rows.params["alpha"]), on(dev, rows.params["beta"])

    def call(x, idx, mask=None):
        return [norm.apply(x, source, alpha=alpha[idx], beta=beta[idx], own_basis=own_basis, mask=mask)]

    # (the masked call copies a tile whose SOURCE row holds a NaN; a NaN factor is no such row, so it runs: every row is "plain")
    (out,) = hold_rows(dev, f"jitter {'own' if own_basis else 'normalised'}", f"H&E jitter {'own' if own_basis else 'normalised'}", kind, layout, rows, call,
                       [ps.he_factors64(kind, own_basis)], top=255.0, bound=TOL_255)
    n = len(rows)
    x = ps.images(kind, layout, n).to(dev)
    ones = torch.ones((n,) + ps.LAYOUTS[layout], dtype=torch.uint8, device=dev)
    finite = torch.from_numpy(np.isfinite(rows.params["alpha"]).all(axis=1) & np.isfinite(rows.params["beta"]).all(axis=1)).to(dev)
    assert same_bits(call(x, np.arange(n), mask=ones)[0][finite], out[finite]), (kind, layout, "the masked jitter with all ones is not the unmasked one")
    if not own_basis:      # 4: the identity factors give the bits of the call without factors
        t = rows.index("identity")
        assert same_bits(out[t:t + 1], norm.apply(x[t:t + 1].clone(), source)), (kind, layout, "the identity factors are not the apply without factors")


# ------------------------------------------------------------------------------------------------ three-stain bases: sx_deconv_*
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", ["apply", "target", "separate", "combine"])
def test_bases(dev, entry, kind, layout):
    """The bases go in as DEVICE tensors, one per tile (the CPU path refuses a singular or a NaN basis)."""
    rows = ps.bases()
    ref = ps.bases64(kind)
    defined = ps.basis_defined(rows)
    basis, target = on(dev, rows.params["basis"]), on(dev, rows.params["target"])
    n = len(rows)
    a, b = torch.tensor([dn.ALPHA] * n, dtype=torch.float32, device=dev), torch.tensor([dn.BETA] * n, dtype=torch.float32, device=dev)
    conc_in = ps.combine_input(kind)[0]      # (3, 1, P)
    h, w = ps.LAYOUTS[layout]

    def deconv(idx, last=False):
        return ColorDeconvolution(basis[idx], target=target[idx] if entry == "target" else None, device=dev, channel_axis=-1 if last else 1)

    def call(x, idx, mask=None, last=False):
        d = deconv(idx, last)
        if entry == "separate":
            got = d.separate(x, stains=True, concentrations=True)
            return [nchw(got.images[s], last) for s in range(3)] + [nchw(got.concentrations, last)]
        if entry == "combine":      # (x: the tiles' pixel INDEX carried as concentrations -- see below)
            return [nchw(d.combine(x, out_dtype=ps.DTYPES[kind]), last)]
        return [nchw(d.apply(x, a[idx], b[idx], mask=mask) if entry == "apply" else d.apply(x, mask=mask), last)]

    if entry == "combine":
        index = ps.tile_index(layout, n)
        c_tiles = on(dev, np.ascontiguousarray(conc_in[:, 0, :][:, index].transpose(1, 0, 2)).reshape(n, 3, h, w))
        out = call(c_tiles, np.arange(n))[0]
        inside_t = torch.from_numpy(rows.inside).to(dev)
        note("bases combine", kind, check_tiles(f"combine {kind} {layout}", out[inside_t], ps.spread(ref["combine"], layout)[rows.inside], np.ones((int(rows.inside.sum()), h, w), dtype=bool), TOL_255,
                                              range_everywhere=False))
        in_range(f"combine {kind} {layout}", out, 255.0, torch.from_numpy(defined))
        for t in range(n):
            assert same_bits(call(c_tiles[t:t + 1].clone(), np.array([t]))[0][0], out[t]), (kind, layout, rows.names[t])
        assert same_bits(call(unaligned_copy(c_tiles), np.arange(n))[0], out)
        assert same_bits(call(c_tiles.permute(0, 2, 3, 1).contiguous(), np.arange(n), last=True)[0], out), (kind, layout, "channels last: other bits")
        return
    raws = [np.ascontiguousarray(ref["stains"][:, s]) for s in range(3)] + [("conc", ref["conc"])] if entry == "separate" else [ref[entry]]
    outs = hold_rows(dev, f"deconv {entry}", f"bases {entry}", kind, layout, rows, call, raws, top=255.0, bound=TOL_255, defined=defined,
                     masked=entry != "separate", nan_rule=lambda x_cpu, k: background_expected(x_cpu, False), nan_keys=("basis", "target") if entry == "target" else ("basis",))
    x_last = ps.images(kind, layout, n, channels_last=True).to(dev)
    for got, want in zip(call(x_last, np.arange(n), last=True), outs):
        assert same_bits(got, want), (entry, kind, layout, "channels last: other bits")
    if entry == "separate":      # quantify counts the bits separate writes, per tile and pooled, on every row with defined values
        k, z = vs.QUANTIFY_BINNING
        sel = np.flatnonzero(defined)
        x = ps.images(kind, layout, n).to(dev)[torch.from_numpy(sel).to(dev)].contiguous()
        d = deconv(sel)
        counts, sums, pixels = qn.histogram_of(outs[3][torch.from_numpy(sel).to(dev)].cpu().numpy(), k, z)
        for got, want in ((d.quantify(x, bin_log2=k, zero_bin=z), (counts, sums, pixels)), (d.quantify(x, pooled=True, bin_log2=k, zero_bin=z), qn.pooled(counts, sums, pixels))):
            assert np.array_equal(got.counts.cpu().numpy(), want[0]) and np.array_equal(got.sums.cpu().numpy(), want[1]) and np.array_equal(got.pixels.cpu().numpy(), want[2]), (kind, layout)
        assert (pixels[rows.inside[sel]] == h * w).all(), "every pixel of a row inside the domain is counted"


# ------------------------------------------------------------------------------------------------ Reinhard statistics
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("reference", list(ps.reinhard_references()))
def test_reinhard(dev, reference, kind, layout):
    rows = ps.reinhard()
    rm, rs = ps.reinhard_references()[reference]
    norm = Reinhard(device=dev, backend="torch_hip")
    norm._reference_mean, norm._reference_std = on(dev, rm), on(dev, rs)
    norm._is_fitted = True
    mean, std = on(dev, rows.params["mean"]), on(dev, rows.params["std"])

    def call(x, idx, mask=None):
        return [norm.apply(x, (mean[idx], std[idx]), mask=mask)]

    hold_rows(dev, f"reinhard, reference {reference}", "Reinhard", kind, layout, rows, call, [ps.reinhard64(kind, reference)], top=1.0, bound=vs.REINHARD_TOL,
              masked=True, nan_rule=lambda x_cpu, k: x_cpu)


# ------------------------------------------------------------------------------------------------ lookup tables
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_tables(dev, kind, layout):
    """Exact arithmetic: EVERY row has the bits of the restatement, whose rule for entries outside 0..255 is the header's."""
    rows = ps.tables()
    n = len(rows)
    luts = on(dev, rows.params["lut"])
    for last in (False, True):
        norm = HistogramMatching(device=dev, backend="torch_hip", channel_axis=-1 if last else 1)
        ref_tile = synth.as_dtype(synth.reference_tile(64, 64), ps.DTYPES[kind])
        norm.fit((ref_tile.permute(0, 2, 3, 1).contiguous() if last else ref_tile).to(dev))
        x_cpu = ps.images(kind, layout, n, channels_last=last)
        x = x_cpu.to(dev)
        want = ps.tables_expected(kind, layout, slice(0, n), channels_last=last)
        out = norm.apply(x, luts)
        differ = (bits(out.cpu()) != bits(want)).reshape(n, -1).any(dim=1)
        assert not bool(differ.any()), (kind, layout, last, [rows.names[i] for i in np.flatnonzero(differ.numpy())])
        in_range(f"tables {kind} {layout}", out, 1.0)
        for t in range(n):
            assert same_bits(norm.apply(x[t:t + 1].clone(), luts[t:t + 1])[0], out[t]), (kind, layout, last, rows.names[t])
        assert same_bits(norm.apply(unaligned_copy(x), luts), out)
        h, w = ps.LAYOUTS[layout]
        assert same_bits(norm.apply(x, luts, mask=torch.ones((n, h, w), dtype=torch.uint8, device=dev)), out), (kind, layout, last, "the masked call with all ones is not the unmasked call")
        if kind == "u8":      # 4: the identity table on uint8 is a copy
            assert same_bits(out[rows.index("identity")].cpu(), x_cpu[rows.index("identity")])


# ------------------------------------------------------------------------------------------------ luminosity rows
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_luminosity(dev, kind, layout):
    rows = ps.luminosity()
    std = LuminosityStandardizer(device=dev)
    y = on(dev, rows.params["y"])
    copied = ps.luminosity_copied(rows)
    (out,) = hold_rows(dev, "luminosity", "luminosity", kind, layout, rows, lambda x, idx, mask=None: [std.apply(x, y[idx])], [ps.luminosity64(kind)], top=1.0, bound=vs.LUMINOSITY_TOL,
                       held=rows.inside & ~copied)
    # 4: rows that are NaN, have L_p <= 0 or equal 1 are copied bit for bit
    x_cpu = ps.images(kind, layout, len(rows))
    sel = torch.from_numpy(copied)
    assert int(copied.sum()) >= 6 and same_bits(out.cpu()[sel], x_cpu[sel]), (kind, layout, [rows.names[i] for i in np.flatnonzero(copied)])


def test_print_the_worst_errors():
    """Not a check: the figures DESIGN.md 5e quotes, per family and float type (run the file with ``-s``)."""
    for (family, kind), worst in sorted(WORST.items()):
        print(f"worst |out - float64| inside the domain: {family:<32} {kind:<5} {worst:.3e}")
