"""Every input value through the stain kernels, against float64 (the sets and the references: tests/_value_sweep.py; what they rely on:
tests/test_value_sweep_cpu.py; the sibling of tests/test_value_sweep_gpu.py, whose helpers it imports).  The entry points are the public
ones that take their statistics as arguments: ``Macenko.separate(source=...)`` (sx_macenko_separate_apply), ``Macenko.apply(..., alpha=,
beta=)`` (sx_macenko_apply with factors), ``ColorDeconvolution.apply`` / ``separate`` / ``combine`` / ``quantify`` (sx_deconv_*) and
``LuminosityStandardizer.apply`` (sx_luminosity_apply).

Sets: A (all 2^24 uint8 colours, ONCE: the pack layout), A_small (uint8 through the single-element path: an odd layout only), B (every
16-bit pattern of bf16 / f16) and C (float32) in both layouts; ``combine`` runs the concentration set K.  Every call runs aligned and one
element off a 16-byte address, and channels-last where the entry point has that form.

* Concentrations inside the domain are within CONC_TOL of float64; images within TOL_255 (float32), plus half an ulp (bf16 / f16); uint8
  equals the truncated float64 value except within the bound of an integer, where one level is allowed -- check_against_float64's rules.
* Outside the domain -- finite or not -- every IMAGE element is finite and in range (concentrations there are unspecified), and
  replacing those pixels by 0.5 grey changes no bit of any in-domain pixel.  A masked call (mask = the in-domain pixels) gives the
  masked-in pixels the unmasked call's bits and the masked-out ones the documented background.
* quantify: counts, sums and pixels equal tests/_quantify_numpy.py's histogram of the bits ``separate`` writes, exactly; and against
  float64 a pixel is in its bin, or -- NaN / Inf member, 255 x + 1 <= 0 -- in none.
* Luminosity: 1e-4 on [0, 1] inside [0, 1]; a row of Y_p = 1 (gain 1) and a NaN row copy the tile bit for bit; outside the domain only
  independence (the header leaves the value a NaN pixel becomes unspecified).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import ColorDeconvolution, LuminosityStandardizer
from tests import _deconv_numpy as dn
from tests import _quantify_numpy as qn
from tests import _value_sweep as vs
from tests.test_apply_gpu import TOL_255
from tests.test_hm_slide_gpu import bits, same_bits, unaligned_copy
from tests.test_macenko_mask_gpu import background_expected
from tests.test_separate_apply_gpu import no_stain_level
from tests.test_value_sweep_gpu import forms, macenko_normaliser

pytestmark = pytest.mark.gpu

SETS = {"A": vs.set_a, "A_small": vs.set_a_small, "B_bf16": lambda: vs.set_b(torch.bfloat16), "B_f16": lambda: vs.set_b(torch.float16), "C": vs.set_c}
HALVES = (torch.bfloat16, torch.float16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def nchw(t: torch.Tensor, last: bool) -> torch.Tensor:
    """A channels-last result (..., H, W, 3) as (..., 3, H, W)."""
    return t.movedim(-1, -3).contiguous() if last else t


def check_tiles(what, out: torch.Tensor, raw: np.ndarray, dom: np.ndarray, bound: float, top: float = 255.0, range_everywhere: bool = True) -> float:
    """check_against_float64's rules (tests/test_value_sweep_gpu.py) on tiles: ``out`` (N, 3, H, W) of any output type against ``raw``, the
    float64 value on the scale 0..``top`` BEFORE the clip, on the pixels of ``dom`` (N, H, W).  Returns the worst error.
    The float64 reference is compared where the result lives (the arithmetic of the numpy rules, in torch float64 on the device)."""
    assert tuple(out.shape) == raw.shape, (what, tuple(out.shape), raw.shape)
    raw = torch.from_numpy(np.ascontiguousarray(raw)).to(out.device)
    dom = torch.from_numpy(np.ascontiguousarray(dom)).to(out.device)[:, None].expand(raw.shape)
    ref = raw.clamp(0.0, top)      # (a NaN stays a NaN)
    zero = torch.zeros((), dtype=torch.float64, device=out.device)
    if out.dtype == torch.uint8:
        got = out.to(torch.int16)
        to_levels = 255.0 / top
        levels, near_by = raw * to_levels, bound * to_levels
        near = ((levels - levels.round()).abs() <= near_by) & (levels >= -near_by) & (levels <= 255.0 + near_by)      # vs.near_integer
        want = (torch.where(dom, ref, zero) * to_levels).trunc().to(torch.int16)
        strict, loose = dom & ~near, dom & near
        off_strict = int(((got != want) & strict).sum())
        assert off_strict == 0, (what, off_strict)
        worst = int(((got - want).abs() * loose).max())
        assert worst <= 1, (what, worst)
        print(f"{what}: uint8 equals trunc(float64) on {int(strict.sum())} elements; {int(((got != want) & loose).sum())} of {int(loose.sum())} within {near_by:.3e} of an integer differ, by one level")
        return float(worst)
    got = out.double()
    if range_everywhere:      # outside the domain, finite or not: a finite value of the output range
        assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= top, (what, "out of range")
    allowed = half_ulp(ref, out.dtype) + bound if out.dtype in HALVES else bound
    err = torch.where(dom, (got - ref).abs(), zero)
    over = torch.where(dom, err - allowed, zero - 1.0)
    worst = float(err.max())      # (a NaN in the domain is the maximum, and fails below)
    print(f"{what}: max |out - float64| = {worst:.3e} on {int(dom.sum())} in-domain elements (bound {bound:.3e}" + (" + half an ulp" if out.dtype in HALVES else "") + f"), worst excess {float(over.max()):.3e}")
    assert float(over.max()) <= 0.0, (what, worst)
    return worst


def half_ulp(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """vs.half_ulp on a float64 tensor: half a unit in the last place of ``dtype`` at the reference value.  The exponent comes from frexp,
    which is exact; numpy's log2 rounds the double just below a power of two up to it, where this is the smaller, stricter value."""
    mantissa_bits, e_min = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = (torch.frexp(ref.abs())[1] - 1).clamp_min(e_min).double()      # floor(log2 |ref|), not below the type's smallest normal exponent
    e = torch.where(torch.isfinite(ref) & (ref != 0), e, torch.full_like(e, float(e_min)))
    return 0.5 * torch.exp2(e - mantissa_bits)


def check_concentrations(what, conc: torch.Tensor, ref: np.ndarray, dom: np.ndarray) -> float:
    assert conc.dtype == torch.float32 and tuple(conc.shape) == ref.shape, what
    ref = torch.from_numpy(np.ascontiguousarray(ref)).to(conc.device)
    sel = torch.from_numpy(np.ascontiguousarray(dom)).to(conc.device)[:, None].expand(ref.shape)
    worst = float(torch.where(sel, (conc.double() - ref).abs(), torch.zeros((), dtype=torch.float64, device=conc.device)).max())
    print(f"{what}: max |C - float64| = {worst:.3e} on {int(sel.sum())} in-domain values (bound {vs.CONC_TOL:.1e})")
    assert worst <= vs.CONC_TOL, (what, worst)      # (a NaN in the domain is the maximum, and fails here too)
    return worst


def same_inside(a: torch.Tensor, b: torch.Tensor, dom: torch.Tensor) -> bool:
    """The bits of two results on the pixels of ``dom`` (N, H, W); the results are (N, K, H, W) or (S, N, K, H, W).  Compared where they are."""
    a, b = bits(a), bits(b)
    dom = dom.to(a.device)
    sel = (dom[:, None] if a.dim() == 4 else dom[None, :, None]).expand(a.shape)
    return a.shape == b.shape and not bool(((a != b) & sel).any())


class Checked:
    """The results already held to float64, on the device.  A later form of the same call (one element off a 16-byte address, channels
    last) that returns the same BITS has passed the same check; one that does not is checked in full."""

    def __init__(self):
        self.held: dict = {}

    def __call__(self, key, out: torch.Tensor, check) -> None:
        first = self.held.get(key)
        if first is not None and first.dtype == out.dtype and first.shape == out.shape and torch.equal(bits(first), bits(out)):
            return
        check()
        self.held.setdefault(key, out)


def again_form(form: str, clean: torch.Tensor) -> torch.Tensor:
    return clean if form == "aligned" else unaligned_copy(clean)


# ------------------------------------------------------------------------------------------------ 1. separation with a given basis
@pytest.mark.parametrize("own_basis", [True, False], ids=["own", "normalised"])
@pytest.mark.parametrize("name", list(SETS))
def test_separation_against_float64(dev, name, own_basis):
    """Measured with the image coefficients of separate_apply_kernel's fold (``h``, ``e``) cut to bf16 in a scratch build: the test fails
    on every set tried, own basis and normalised -- the H image of set C is 5.6 / 3.7 levels from float64 (bound 2.55e-2), that of B bf16
    3.0 / 2.6 beyond its bound, 223 774 / 14 508 uint8 elements of A_small are off their level."""
    sweep = SETS[name]()
    norm, source = macenko_normaliser(dev)
    st = vs.statistics()
    scale = 1.0 if own_basis else (st["tmc"].astype(np.float64) / st["max_c"].astype(np.float64)).reshape(1, 2, 1, 1)
    mode = "own" if own_basis else "normalised"
    dom_px = sweep.macenko_domain
    for layout in vs.stain_layouts(sweep):
        dom = sweep.spread(layout, dom_px)
        dom_t = torch.from_numpy(dom)
        conc_ref = sweep.spread(layout, sweep.separation["conc"]) * scale
        raws = [sweep.spread(layout, np.ascontiguousarray(sweep.separation[mode][:, s])) for s in range(2)]
        clean = sweep.images(layout, replace=~dom_px).to(dev)
        checked = Checked()
        for form, x in forms(sweep.images(layout).to(dev)):
            what = f"separate {mode} {name} {layout.name} {form}"
            got = norm.separate(x, source=source, own_basis=own_basis, stains=True, concentrations=True)
            checked("C", got.concentrations, lambda: check_concentrations(what, got.concentrations, conc_ref, dom))
            for image, raw, stain in ((got.hematoxylin, raws[0], "H"), (got.eosin, raws[1], "E")):
                assert image.dtype == sweep.dtype, what
                checked(stain, image, lambda: check_tiles(f"{what} {stain}", image, raw, dom, TOL_255))
            if not bool(dom.all()):      # independence: the out-of-domain pixels replaced by 0.5 grey
                again = norm.separate(again_form(form, clean), source=source, own_basis=own_basis, stains=True, concentrations=True)
                for a, b in ((got.concentrations, again.concentrations), (got.hematoxylin, again.hematoxylin), (got.eosin, again.eosin)):
                    assert same_inside(a, b, dom_t), (what, "a pixel outside the domain changed another pixel")
                assert torch.isfinite(again.concentrations).all() and torch.isfinite(again.hematoxylin.float()).all()


# ------------------------------------------------------------------------------------------------ 2. the jitter with a given basis
@pytest.mark.parametrize("own_basis", [False, True], ids=["normalised", "own"])
@pytest.mark.parametrize("name", list(SETS))
def test_given_basis_jitter_against_float64(dev, name, own_basis):
    sweep = SETS[name]()
    norm, source = macenko_normaliser(dev)
    dom_px = sweep.macenko_domain
    for layout in vs.stain_layouts(sweep):
        dom = sweep.spread(layout, dom_px)
        dom_t = torch.from_numpy(dom)
        clean = sweep.images(layout, replace=~dom_px).to(dev)
        for shift in vs.row_shifts(layout, len(vs.JITTER)):
            ref = sweep.jitter(layout, own_basis, shift)
            alpha, beta = torch.from_numpy(ref["alpha"]).to(dev), torch.from_numpy(ref["beta"]).to(dev)
            identity = torch.from_numpy(ref["pair"] == 0)
            checked = Checked()
            for form, x in forms(sweep.images(layout).to(dev)):
                what = f"jitter {'own' if own_basis else 'normalised'} {name} {layout.name} shift {shift} {form}"
                out = norm.apply(x, source, alpha=alpha, beta=beta, own_basis=own_basis)
                assert out.dtype == sweep.dtype, what
                checked("out", out, lambda: check_tiles(what, out, ref["raw"], dom, TOL_255))
                if not own_basis and bool(identity.any()):      # alpha = 1, beta = 0: the apply without factors, bit for bit
                    plain = norm.apply(x, source)
                    assert same_bits(out[identity.to(dev)].cpu(), plain[identity.to(dev)].cpu()), (what, "the identity row is not the apply without factors")
                if not bool(dom.all()):
                    again = norm.apply(again_form(form, clean), source, alpha=alpha, beta=beta, own_basis=own_basis)
                    assert same_inside(out, again, dom_t), (what, "a pixel outside the domain changed another pixel")
                    assert torch.isfinite(again.float()).all()


# ------------------------------------------------------------------------------------------------ 3. deconvolution
def deconv_factors(n: int, dev) -> tuple[torch.Tensor, torch.Tensor]:
    return torch.tensor([dn.ALPHA] * n, dtype=torch.float32, device=dev), torch.tensor([dn.BETA] * n, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("entry", ["apply", "target", "separate"])
@pytest.mark.parametrize("basis", vs.DECONV_NAMES)
@pytest.mark.parametrize("name", list(SETS))
def test_deconvolution_against_float64(dev, name, basis, entry):
    sweep = SETS[name]()
    ref = sweep.deconv(basis)
    dom_px = sweep.macenko_domain
    for layout in vs.stain_layouts(sweep):
        dom = sweep.spread(layout, dom_px)
        dom_t = torch.from_numpy(dom)
        a, b = deconv_factors(layout.n, dev)
        if entry == "separate":
            conc_ref = sweep.spread(layout, ref["conc"])
            raws = [sweep.spread(layout, np.ascontiguousarray(ref["stains"][:, s])) for s in range(3)]
        else:
            raw = sweep.spread(layout, ref[entry])
        checked = Checked()
        for last in (False, True):
            deconv = ColorDeconvolution(basis, target=vs.OTHER_BASIS[basis] if entry == "target" else None, device=dev, channel_axis=-1 if last else 1)
            clean = sweep.images(layout, channels_last=last, replace=~dom_px).to(dev)

            def run(x):
                if entry == "separate":
                    got = deconv.separate(x, stains=True, concentrations=True)
                    return [nchw(got.concentrations, last), nchw(got.images, last)]
                return [nchw(deconv.apply(x, a, b) if entry == "apply" else deconv.apply(x), last)]

            for form, x in forms(sweep.images(layout, channels_last=last).to(dev)):
                what = f"deconv {basis} {entry} {name} {layout.name} {'NHWC' if last else 'NCHW'} {form}"
                got = run(x)
                if entry == "separate":
                    checked("C", got[0], lambda: check_concentrations(what, got[0], conc_ref, dom))
                    assert got[1].dtype == sweep.dtype and got[1].shape[0] == 3, what
                    for s in range(3):
                        checked(s, got[1][s], lambda: check_tiles(f"{what} image {s}", got[1][s], raws[s], dom, TOL_255))
                else:
                    assert got[0].dtype == sweep.dtype, what
                    checked("out", got[0], lambda: check_tiles(what, got[0], raw, dom, TOL_255))
                    if sweep.dtype == torch.uint8 and entry == "apply":
                        # uint8 -> bf16 / f16: by the header the bits of the uint8 result cast to the type (every level 0..255 is a value
                        # of both types), so the uint8 rule above holds for them -- not float64 rounded to the type: the level is truncated
                        for half in HALVES:
                            out = deconv._engine(dev).apply(x, *deconv._bases_on(dev), alpha=a, beta=b, out_dtype=half, channels_last=last)
                            assert same_bits(nchw(out, last), got[0].to(half)), (what, half, "not the uint8 result cast to the type")
                if not bool(dom.all()):
                    for one, other in zip(got, run(again_form(form, clean))):
                        assert same_inside(one, other, dom_t), (what, "a pixel outside the domain changed another pixel")
                        assert torch.isfinite(other.float()).all()


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32, torch.bfloat16, torch.float16], ids=["u8", "f32", "bf16", "f16"])
@pytest.mark.parametrize("basis", vs.DECONV_NAMES)
def test_combine_against_float64(dev, basis, out_dtype):
    """Concentrations that are no separation's output: large, negative, +-Inf, NaN, +-FLT_MAX (tests/_value_sweep.py: concentration_set)."""
    sweep = vs.concentration_set()
    dom_px = vs.combine_domain(sweep)
    for layout in sweep.layouts.values():
        dom = sweep.spread(layout, dom_px)
        dom_t = torch.from_numpy(dom)
        raw = sweep.spread(layout, vs.combine64(basis))
        checked = Checked()
        for last in (False, True):
            deconv = ColorDeconvolution(basis, device=dev, channel_axis=-1 if last else 1)
            clean = sweep.images(layout, channels_last=last, replace=~dom_px).to(dev)
            for form, c in forms(sweep.images(layout, channels_last=last).to(dev)):
                what = f"combine {basis} {layout.name} {'NHWC' if last else 'NCHW'} {form}"
                out = nchw(deconv.combine(c, out_dtype=out_dtype), last)
                assert out.dtype == out_dtype, what
                checked("out", out, lambda: check_tiles(what, out, raw, dom, TOL_255))
                again = nchw(deconv.combine(again_form(form, clean), out_dtype=out_dtype), last)
                assert same_inside(out, again, dom_t), (what, "a concentration outside the domain changed another pixel")


# ------------------------------------------------------------------------------------------------ 4. quantify
@pytest.mark.parametrize("basis", vs.DECONV_NAMES)
@pytest.mark.parametrize("name", list(SETS))
def test_quantify_counts_the_bits_of_separate_and_the_float64_bins(dev, name, basis):
    """Measured with the finiteness test of deconv_quantify_kernel dropped in a scratch build (a NaN then lands in bin 0): the counts no
    longer equal the histogram of separate's bits on B bf16, B f16 and C, both bases; the uint8 sets, which hold no such pixel, pass."""
    sweep = SETS[name]()
    k, z = vs.QUANTIFY_BINNING
    ref = sweep.deconv(basis)["conc"]
    x64 = sweep.x32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        unit = x64 * 255.0 + 1.0
        not_finite_px = ~np.isfinite(x64).all(axis=1)
        pole_px = (unit <= -vs.POLE_BAND).any(axis=1)                  # a member with 255 x + 1 <= 0: no logarithm
        undecided_px = (np.abs(unit) < vs.POLE_BAND).any(axis=1)
    for layout in vs.stain_layouts(sweep):
        dom = sweep.spread(layout, sweep.macenko_domain)
        none = sweep.spread(layout, (not_finite_px | pole_px) & ~undecided_px)
        conc64 = sweep.spread(layout, ref)
        with np.errstate(invalid="ignore"):      # (outside the domain a concentration may be Inf or NaN)
            sure = np.broadcast_to(dom[:, None], conc64.shape) & ~qn.near_edge(conc64, k)
            want_bin = np.clip(np.floor(np.where(sure, conc64, 0.0) * 2.0**k).astype(np.int64) + z, 0, qn.BINS - 1)
        first = None
        for last in (False, True):
            deconv = ColorDeconvolution(basis, device=dev, channel_axis=-1 if last else 1)
            for form, x in forms(sweep.images(layout, channels_last=last).to(dev)):
                what = f"quantify {basis} {name} {layout.name} {'NHWC' if last else 'NCHW'} {form}"
                conc_dev = nchw(deconv.separate(x, stains=False, concentrations=True).concentrations, last)
                fresh = first is None or not same_bits(first[0], conc_dev)
                if fresh:      # (the restated histogram of the same bits is the same histogram)
                    conc32 = conc_dev.cpu().numpy()
                    first = (conc_dev, conc32, qn.histogram_of(conc32, k, z))
                _, conc32, (counts, sums, pixels) = first
                per_tile, pooled = deconv.quantify(x, bin_log2=k, zero_bin=z), deconv.quantify(x, pooled=True, bin_log2=k, zero_bin=z)
                for got, want in ((per_tile, (counts, sums, pixels)), (pooled, qn.pooled(counts, sums, pixels))):
                    assert np.array_equal(got.counts.cpu().numpy(), want[0]) and np.array_equal(got.sums.cpu().numpy(), want[1]) and np.array_equal(got.pixels.cpu().numpy(), want[2]), what
                if not fresh:      # (the same bits again: they have been held to float64)
                    continue
                counted = np.isfinite(conc32).all(axis=1)
                assert not counted[none].any(), (what, "a pixel with a NaN / Inf member, or beyond the pole, is counted", int(counted[none].sum()))
                assert counted[dom].all(), (what, "an in-domain pixel is not counted")
                with np.errstate(invalid="ignore", over="ignore"):
                    got_bin = qn.bins_of(np.where(sure, conc32, np.float32(0.0)), k, z)
                assert np.array_equal(got_bin[sure], want_bin[sure]), (what, int((got_bin != want_bin)[sure].sum()))
                print(f"{what}: counts, sums and pixels equal the histogram of separate's bits ({int(pixels.sum())} of {counted.size} pixels counted, {int(none.sum())} with a "
                      f"non-finite member or beyond the pole in no count); {int(sure.sum())} in-domain values in their float64 bin, {int((~sure).sum() - 3 * (~dom).sum())} near an edge")


# ------------------------------------------------------------------------------------------------ 5. masks as independence
@pytest.mark.parametrize("name", list(SETS))
def test_masked_calls_are_the_unmasked_call_inside_and_background_outside(dev, name):
    """mask = the in-domain pixels, pack layout (set A_small has none: its odd layout), planar tiles: the masked calls refuse
    channels-last.  A masked-out pixel holds no stain in a separation (concentrations +0.0, both images the level of zero concentration,
    240) and its own input level after ``ColorDeconvolution.apply`` (compared where the member is not a NaN)."""
    sweep = SETS[name]()
    norm, source = macenko_normaliser(dev)
    layout = sweep.layouts.get("packs", next(iter(sweep.layouts.values())))
    dom = torch.from_numpy(sweep.spread(layout, sweep.macenko_domain))
    mask = dom.to(torch.uint8).to(dev)
    images = sweep.images(layout)
    x = images.to(dev)
    outside = (~dom)[:, None].expand(layout.n, 3, layout.h, layout.w)
    level = no_stain_level(sweep.dtype, False)
    for own_basis in (True, False):
        what = f"masked separate {name} own_basis={own_basis}"
        plain = norm.separate(x, source=source, own_basis=own_basis, stains=True, concentrations=True)
        masked = norm.separate(x, source=source, own_basis=own_basis, stains=True, concentrations=True, mask=mask)
        for a, b in ((plain.concentrations, masked.concentrations), (plain.hematoxylin, masked.hematoxylin), (plain.eosin, masked.eosin)):
            assert same_inside(a, b, dom), what
        assert not bool(masked.concentrations.cpu().view(torch.int32)[outside[:, :2]].any()), (what, "a masked-out concentration is not +0.0")
        for image in (masked.hematoxylin, masked.eosin):
            assert image.dtype == level.dtype and bool((bits(image.cpu())[outside] == bits(level.reshape(1))[0]).all()), (what, "a masked-out pixel is not the 240 level")
    deconv = ColorDeconvolution("hed", device=dev)
    a, b = deconv_factors(layout.n, dev)
    plain, masked = deconv.apply(x, a, b), deconv.apply(x, a, b, mask=mask)
    assert same_inside(plain, masked, dom), f"masked deconv apply {name}"
    copied = outside & ~torch.isnan(images.float())
    # (bits, but for the sign of a zero level: the clamp of -0.0 to [0, 255] is level 0 whichever zero it returns -- fmaxf gives +0.0 on
    # the device, torch.clamp keeps -0.0 in background_expected; set C holds one such member under the mask)
    want = background_expected(images, False)
    differ = copied & (bits(masked.cpu()) != bits(want)) & ~((masked.cpu() == 0) & (want == 0))
    examples = [(float(v), float(g)) for v, g in zip(images[differ][:8].float(), masked.cpu()[differ][:8].float())]
    assert not bool(differ.any()), (f"masked deconv apply {name}: a masked-out pixel is not its input level", int(differ.sum()), examples)
    print(f"masks {name}: {int(dom.sum())} pixels masked in, {int((~dom).sum())} masked out")


# ------------------------------------------------------------------------------------------------ 6. the luminosity apply pass
LUMINOSITY_ROWS = vs.LUMINOSITY_Y + (float("nan"),)      # L_p = 30, 75, 100 (gain 1: copied) and a row without a percentile (copied)


@pytest.mark.parametrize("name", list(SETS))
def test_luminosity_apply_against_float64(dev, name):
    sweep = SETS[name]()
    std = LuminosityStandardizer(device=dev)
    dom_px = sweep.luminosity_domain
    rows = len(LUMINOSITY_ROWS)
    for layout in vs.stain_layouts(sweep):
        dom = sweep.spread(layout, dom_px)
        dom_t = torch.from_numpy(dom)
        images = sweep.images(layout)
        clean = sweep.images(layout, replace=~dom_px).to(dev)
        for shift in vs.row_shifts(layout, rows):
            row = (np.arange(layout.n) + shift) % rows
            mapped = row < 2
            estimate = torch.tensor([LUMINOSITY_ROWS[r] for r in row], dtype=torch.float32, device=dev)
            raw = np.zeros((layout.n, 3, layout.h, layout.w))
            for r in (0, 1):
                if (row == r).any():
                    raw[row == r] = sweep.spread(layout, np.ascontiguousarray(sweep.luminosity["raw"][:, r]))[row == r]
            checked = Checked()
            for form, x in forms(images.to(dev)):
                what = f"luminosity {name} {layout.name} shift {shift} {form}"
                out = std.apply(x, estimate)
                assert out.dtype == sweep.dtype and out.shape == x.shape, what
                if mapped.any():
                    checked("out", out, lambda: check_tiles(what, out[torch.from_numpy(mapped).to(dev)], raw[mapped], dom[mapped], vs.LUMINOSITY_TOL, top=1.0, range_everywhere=False))
                copied = torch.from_numpy(~mapped)
                assert same_bits(out.cpu()[copied], images[copied]), (what, "a row of gain 1, or a NaN row, does not copy its tile bit for bit")
                if not bool(dom.all()):
                    again = std.apply(again_form(form, clean), estimate)
                    assert same_inside(out, again, dom_t), (what, "a pixel outside the domain changed another pixel")
