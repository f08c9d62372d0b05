"""Blur, JPEG, focus and the two warps on the shapes and parameter rows of tests/_tiled_edges.py: blocks on the 4-pixel pack path that the
tile's edge cuts, every radius of the blur with both sides of every border of the radius rule, the blur's impulse response, every JPEG
quality and the quality rule's corners.  The helpers, the yardsticks and EVERY bound are those of the kernels' own test files, imported:
tests/test_blur_gpu.py (``raw``, ``check`` with BAND / TOL), tests/test_jpeg_gpu.py (bit for bit against tests/_jpeg_numpy.py),
tests/test_focus_gpu.py (exact integers), tests/test_warp_gpu.py and tests/test_elastic_gpu.py (``exact_output``).

The one bound that is new is the impulse response's, REL = 2^-15 relative (3.1e-5; a missing or doubled tap is an error of order 1, and
the blur tests' 1e-4 absolute cannot see the outermost tap, which weighs 3.3e-5 at sigma 4).  It is DERIVED, in units of u = 2^-24, for a
tile of +0.0 with a single 1.0, where each pass returns the taps themselves and an output is fl(w_|dy| * w_|dx|) (plus, where the border
folds several taps onto one pixel, a chain of at most 16 additions of positive terms per pass):
    the exponent   scale = -0.5f / (sigma * sigma): two roundings; (float)(i * i) * scale: one -- 3 u relative on an argument of at most
                   32 in magnitude (the tap R of a sigma on a border: 8 (k + 1)^2 / (k + 0.5)^2 <= 32): 96 u on the exponential;
    expf           2 units in the last place: 4 u -- a tap before the division: 100 u;
    the sum        positive terms, each within 100 u, added in at most 17 steps: 117 u; the division: 1 u -- a tap: 218 u;
    the product    two taps and one rounding: 437 u; the folded chains: 2 x 16 u -- 469 u < 512 u = 2^-15.
The sigma enters the float64 taps exactly.  tests/test_tiled_edges_cpu.py holds a numpy float32 model of the taps, built by the same rule,
to a quarter of REL against the float64 taps (measured: 1.7e-6).  Where the float64 response is exactly 0 the output must be exactly 0.0:
the support is the (2 R + 1)^2 window folded at the borders, no more and no less -- which pins R on both sides of every border of
R = (int)(4 sigma + 0.5).  For an impulse MORE than R from every border the response must be symmetric bit for bit under transposition and
under both reflections about the impulse (at a distance of exactly R the output on the border reads the impulse twice, at -R and, folded,
at +R: the float64 response says the same, and the window is not symmetric).

Measured on an MI355X (the figures this file prints; DESIGN.md 4s and 4w quote them):
    ragged shapes   uint8 0.50002 levels (band 0.503), float16 2.443e-4 and bfloat16 1.953e-3 (the rounding to the type), float32 and
                    float64 3.37e-7 on [0, 1];
    radius sweep    uint8 0.50003 levels, float32 3.68e-7, bfloat16 1.953e-3;
    impulse         worst |out / ref - 1| = 1.55e-6 on both shapes (REL 3.05e-5), no non-zero output outside a support, every unfolded
                    window symmetric bit for bit;
    JPEG            0 differing bytes on every shape, at every quality 1..100 and on every row of the quality rule."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import _native, focus_statistics, synth
from tests import _blur_numpy as bn
from tests import _elastic_numpy as en
from tests import _focus_numpy as fn
from tests import _jpeg_numpy as jn
from tests import _tiled_edges as te
from tests import _warp_numpy as wn
from tests import test_blur_gpu as blur
from tests import test_elastic_gpu as elastic
from tests import test_jpeg_gpu as jpeg
from tests import test_warp_gpu as warp
from tests.test_blur_gpu import CL, DTYPE_IDS, DTYPES, OUT_FLAG, UNIT, nhwc, sig, tiles_of
from tests.test_focus_gpu import LAYOUTS, in_layout, on, words
from tests.test_hsv_gpu import off_by_one
from tests.test_tissue_mask_gpu import unaligned_copy
from tests.test_warp_gpu import BILINEAR, CONSTANT, MIRROR, NEAREST, bits, exact_output, fill_of, rows_t

pytestmark = pytest.mark.gpu

NAN = float("nan")
BLUR_SHAPES, JPEG_SHAPES, FOCUS_SHAPES, WARP_SHAPES = tuple(te.BLUR_SHAPES), tuple(te.JPEG_SHAPES), tuple(te.FOCUS_SHAPES), tuple(te.WARP_SHAPES)
SWEEP_SHAPES = ((9, 36), (66, 100))
SWEEP_DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


def name_of(dtype: torch.dtype) -> str:
    return str(dtype).split(".")[-1]


# ------------------------------------------------------------------ 2. blur
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=te.ids(BLUR_SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_blur_ragged_pack_blocks_against_float64(dev, lib, dtype, shape):
    """Radii 1, 7 and 16, a copy tile and a clamped sigma in one launch; NHWC, the view one element off (single elements on the same
    shape) and a tile alone give the aligned planar call's bits; so do the masked call's two mask paths."""
    sigmas = te.RAGGED_SIGMAS
    x = te.blur_tiles(dtype, shape, len(sigmas))
    xd, s = x.to(dev), sig(sigmas, dev)
    assert shape[1] % 4 == 0 and xd.data_ptr() % 16 == 0      # the pack path
    out = blur.raw(lib, xd, s)
    assert out.dtype == dtype
    blur.check(out.cpu(), x, False, te.blur_reference(dtype, shape, sigmas), sigmas, ("ragged", name_of(dtype), shape))
    assert torch.equal(blur.raw(lib, nhwc(xd), s, CL).permute(0, 3, 1, 2), out), "NHWC"
    assert torch.equal(blur.raw(lib, off_by_one(xd), s), out), "input one element off"
    assert torch.equal(blur.raw(lib, xd, s, out=off_by_one(torch.empty_like(out))), out), "output one element off"
    for t in range(len(sigmas)):
        assert torch.equal(blur.raw(lib, xd[t:t + 1].contiguous(), s[t:t + 1].contiguous()), out[t:t + 1]), t
    ones = torch.ones(len(sigmas), *shape, dtype=torch.uint8, device=dev)
    assert torch.equal(blur.raw(lib, xd, s, mask=ones), out) and torch.equal(blur.raw(lib, xd, s, mask=off_by_one(ones)), out)
    mask = (torch.rand(len(sigmas), *shape, device=dev) < 0.6).to(torch.uint8) * 255
    masked = blur.raw(lib, xd, s, mask=mask)
    assert torch.equal(blur.raw(lib, xd, s, mask=off_by_one(mask)), masked) and torch.equal(blur.raw(lib, off_by_one(xd), s, mask=mask), masked)
    inside = mask.bool().unsqueeze(1).expand_as(xd)
    copied = blur.raw(lib, xd, sig((NAN,), dev))
    assert torch.equal(masked, torch.where(inside, out, copied))


@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=te.ids(SWEEP_SHAPES))
@pytest.mark.parametrize("dtype", SWEEP_DTYPES, ids=[name_of(d) for d in SWEEP_DTYPES])
def test_blur_every_radius_and_both_sides_of_every_border(dev, lib, dtype, shape):
    """One launch, a sigma per tile: every border (k + 0.5) / 4 of the radius rule with its two float32 neighbours, R / 4 for R = 1..16,
    4.0 and the float above it."""
    sigmas = te.radius_sigmas()
    x = te.blur_tiles(dtype, shape, len(sigmas))
    xd, s = x.to(dev), sig(sigmas, dev)
    out = blur.raw(lib, xd, s)
    blur.check(out.cpu(), x, False, te.blur_reference(dtype, shape, sigmas), sigmas, ("radius sweep", name_of(dtype), shape))
    assert torch.equal(blur.raw(lib, off_by_one(xd), s), out)      # single elements: the same bits at every radius
    top = sigmas.index(4.0)
    assert torch.equal(blur.raw(lib, xd[top:top + 1].contiguous(), sig((float(te.above(4.0)),), dev)), out[top:top + 1])      # clamped: the bits of 4.0


@pytest.mark.parametrize("shape", te.IMPULSE_SHAPES, ids=te.ids(te.IMPULSE_SHAPES))
def test_blur_impulse_response_pins_radius_and_taps(dev, lib, shape):
    x, sigmas, places = te.impulse_tiles(shape)
    want = te.impulse_reference(shape)
    xd, s = x.to(dev), sig(sigmas, dev)
    out = blur.raw(lib, xd, s)
    assert out.dtype == torch.float32
    assert torch.equal(blur.raw(lib, off_by_one(xd), s), out) and torch.equal(blur.raw(lib, nhwc(xd), s, CL).permute(0, 3, 1, 2), out)
    got = out.cpu()
    value = got.to(torch.float64).numpy()
    assert np.isfinite(value).all()
    zero = want == 0.0
    stray = int((value[zero] != 0.0).sum())
    ratio = np.abs(value[~zero] / want[~zero] - 1.0)
    worst = float(ratio.max())
    print(f"impulse {shape}: {len(sigmas)} tiles, {int((~zero).sum())} elements in the supports, {stray} non-zero outputs outside them, worst |out / ref - 1| = {worst:.3e} (REL {te.REL:.3e})")
    assert stray == 0, (shape, stray)      # nothing outside the (2 R + 1)^2 window folded at the borders
    assert worst <= te.REL, (shape, worst, [(sigmas[t], places[t]) for t in sorted({int(i) for i in np.argwhere(np.abs(np.where(zero, 0.0, value / np.where(zero, 1.0, want) - 1.0)) > te.REL)[:, 0]})][:8])
    windows = 0
    h, w = shape
    for t, (sigma, triple) in enumerate(zip(sigmas, places)):
        r = bn.radius(sigma)
        for c, (y, col) in enumerate(triple):
            if r >= 1 and min(y, h - 1 - y, col, w - 1 - col) > r:      # no fold inside the window: every entry is fl(w_|dy| * w_|dx|)
                win = got[t, c, y - r:y + r + 1, col - r:col + r + 1].contiguous()
                assert bool((win > 0).all()), (sigma, (y, col))
                for other, what in ((win.t(), "transposed"), (win.flip(0), "upside down"), (win.flip(1), "mirrored")):
                    assert torch.equal(win.view(torch.int32), other.contiguous().view(torch.int32)), (sigma, (y, col), what)
                windows += 1
    print(f"impulse {shape}: {windows} unfolded windows symmetric bit for bit")
    assert windows >= (2 * (len(te.impulse_sigmas()) - 1) if shape == (100, 132) else 4)


# ------------------------------------------------------------------ 3. JPEG
@pytest.mark.parametrize("sub", jpeg.SUBS, ids=jpeg.SUB_IDS)
@pytest.mark.parametrize("shape", JPEG_SHAPES, ids=te.ids(JPEG_SHAPES))
def test_jpeg_ragged_regions_against_the_restatement(dev, lib, shape, sub):
    x = jpeg.tiles_u8(shape)
    xd, q = x.to(dev), jpeg.qs(te.JPEG_QUALITIES, dev)
    assert shape[1] % 4 == 0 and xd.data_ptr() % 16 == 0      # the pack path
    want = jpeg.reference_rows(shape, te.JPEG_QUALITIES, sub)
    out = jpeg.raw(lib, xd, q, sub)
    differing = int((out.cpu() != want).sum())
    print(f"jpeg {shape} subsampling {sub}: {differing} differing bytes of {want.numel()}")
    assert torch.equal(out.cpu(), want), (shape, sub, differing)
    assert torch.equal(out[3], xd[3]) and not torch.equal(out[0], xd[0])
    ones = torch.ones(4, *shape, dtype=torch.uint8, device=dev)
    for dtype in (torch.uint8, torch.float32, torch.bfloat16):
        xt = jpeg.as_dtype(x, dtype).to(dev)
        aligned = jpeg.raw(lib, xt, q, sub)
        assert aligned.dtype == dtype
        assert torch.equal(aligned[:3], out[:3].to(dtype)), (dtype, "levels")      # (an integer up to 255 is exact in every element type)
        assert torch.equal(aligned[3], jpeg.hsv_copy(lib, xt)[3]), (dtype, "copy")      # sx_hsv_apply's copy: a uint8 tile's bytes, a float tile's levels
        assert torch.equal(jpeg.raw(lib, nhwc(xt), q, sub, CL).permute(0, 3, 1, 2), aligned), (dtype, "NHWC")
        assert torch.equal(jpeg.raw(lib, off_by_one(xt), q, sub), aligned), (dtype, "input one element off")
        assert torch.equal(jpeg.raw(lib, xt, q, sub, out=off_by_one(torch.empty_like(aligned))), aligned), (dtype, "output one element off")
        assert torch.equal(jpeg.raw(lib, xt, q, sub, mask=ones), aligned) and torch.equal(jpeg.raw(lib, xt, q, sub, mask=off_by_one(ones)), aligned), (dtype, "all ones")
        for t in range(4):
            assert torch.equal(jpeg.raw(lib, xt[t:t + 1].contiguous(), q[t:t + 1].contiguous(), sub), aligned[t:t + 1]), (dtype, t)


@lru_cache(maxsize=None)
def every_quality_reference(sub: int) -> torch.Tensor:
    return torch.from_numpy(jn.roundtrip(te.jpeg_tiles(te.QUALITY_SHAPE, 100), te.every_quality(), sub))


@pytest.mark.parametrize("sub", jpeg.SUBS, ids=jpeg.SUB_IDS)
def test_jpeg_every_quality(dev, lib, sub):
    """A hundred tiles in one launch, quality t + 1 for tile t: every table the rule can make, on seeded bytes and on real tissue."""
    x = torch.from_numpy(te.jpeg_tiles(te.QUALITY_SHAPE, 100).copy()).to(dev)
    want = every_quality_reference(sub)
    got = jpeg.raw(lib, x, jpeg.qs(te.every_quality(), dev), sub).cpu()
    wrong = [t + 1 for t in range(100) if not torch.equal(got[t], want[t])]
    print(f"jpeg every quality, subsampling {sub}: {int((got != want).sum())} differing bytes of {want.numel()}; qualities that differ: {wrong}")
    assert not wrong, (sub, wrong)
    assert torch.equal(jpeg.raw(lib, off_by_one(x), jpeg.qs(te.every_quality(), dev), sub).cpu(), want)


@pytest.mark.parametrize("sub", jpeg.SUBS, ids=jpeg.SUB_IDS)
def test_jpeg_quality_rule(dev, lib, sub):
    """Finite rows at or above 1 code with min((int)q, 100) -- FLT_MAX is 100 --; NaN, the infinities and everything below 1 leave their
    tile: sx_hsv_apply's copy."""
    tiles = te.jpeg_tiles(te.RULE_SHAPE, len(te.RULE_ROWS))
    x = torch.from_numpy(tiles.copy()).to(dev)
    rows = jpeg.qs(te.RULE_ROWS, dev)
    assert float(rows[te.RULE_ROWS.index(te.FLT_MAX)]) == te.FLT_MAX and bool(torch.isfinite(rows[te.RULE_ROWS.index(3.2e38)]))
    got = jpeg.raw(lib, x, rows, sub)
    by_integer = jpeg.raw(lib, x, jpeg.qs([float(max(q, 1)) for q in te.RULE_QUALITY], dev), sub)
    copied = jpeg.hsv_copy(lib, x)
    assert torch.equal(copied, x)
    for t, (row, quality) in enumerate(zip(te.RULE_ROWS, te.RULE_QUALITY)):
        if quality == 0:
            assert torch.equal(got[t], copied[t]), (row, "is not a copy")
        else:
            assert torch.equal(got[t].cpu(), torch.from_numpy(jn.roundtrip_levels(tiles[t], quality, sub))), (row, quality, "restatement")
            assert torch.equal(got[t], by_integer[t]) and not torch.equal(got[t], x[t]), (row, quality)
    for flags in (UNIT, OUT_FLAG[torch.bfloat16]):      # the copies through the output rule, the coded tiles through it as well
        out = jpeg.raw(lib, x, rows, sub, flags)
        want = torch.where(torch.tensor([q == 0 for q in te.RULE_QUALITY], device=dev).view(-1, 1, 1, 1), jpeg.hsv_copy(lib, x, flags), jpeg.hsv_identity(lib, got, flags))
        assert torch.equal(out, want), flags
    real = jpeg.as_dtype(torch.from_numpy(tiles.copy()), torch.float32).to(dev)
    out = jpeg.raw(lib, real, rows, sub)
    left = torch.tensor([q == 0 for q in te.RULE_QUALITY], device=dev)
    assert torch.equal(out[left], jpeg.hsv_copy(lib, real)[left]) and torch.equal(out[~left], got[~left].to(torch.float32))


# ------------------------------------------------------------------ 4. focus
@pytest.mark.parametrize("shape", FOCUS_SHAPES, ids=te.ids(FOCUS_SHAPES))
@pytest.mark.parametrize("name", ["u8", "f32"])
def test_focus_ragged_pack_blocks(dev, shape, name):
    u8 = torch.from_numpy(fn.tiles_u8(shape).copy())
    x_cpu = u8 if name == "u8" else synth.as_dtype(u8, torch.float32)
    own = fn.as_numpy(x_cpu)
    mask = fn.tiles_mask(shape)
    planar = x_cpu.to(dev)
    assert shape[2] % 4 == 0 and planar.data_ptr() % 16 == 0      # the pack path
    for block in (None, (8, 8), (16, 32)):
        want = fn.as_torch(fn.statistics(own, block))
        for layout in LAYOUTS:
            x, axis = in_layout(planar, layout)
            assert torch.equal(words(focus_statistics(x, block=block, channel_axis=axis)), want), (block, layout)
        want_masked = fn.as_torch(fn.statistics(own, block, mask))
        m = on(dev, mask)
        assert m.data_ptr() % 4 == 0 and unaligned_copy(m).data_ptr() % 4 != 0
        assert torch.equal(words(focus_statistics(planar, block=block, mask=m)), want_masked), (block, "mask")
        assert torch.equal(words(focus_statistics(planar, block=block, mask=unaligned_copy(m))), want_masked), (block, "mask one byte off")
        assert torch.equal(words(focus_statistics(unaligned_copy(planar), block=block, mask=m)), want_masked), (block, "tiles one element off")
        assert not torch.equal(want_masked, want)
    pooled = fn.as_torch(fn.statistics(own, None, None, True))
    for layout in LAYOUTS:
        x, axis = in_layout(planar, layout)
        assert torch.equal(words(focus_statistics(x, pooled=True, channel_axis=axis)), pooled), layout
    assert torch.equal(words(focus_statistics(planar, pooled=True, mask=on(dev, mask))), fn.as_torch(fn.statistics(own, None, mask, True)))


# ------------------------------------------------------------------ 5. the warps' copy path
def flag_sets(dtype: torch.dtype) -> tuple:
    return (0, UNIT, OUT_FLAG[torch.bfloat16]) if dtype == torch.uint8 else (0, UNIT)


def warp_calls(lib, dev, shape):
    """(name, call(x, rows, interpolation, border, fill, flags) -> out) for sx_affine_warp and for sx_elastic_warp with a non-zero grid."""
    cell = 16
    grids = elastic.grids_t(en.test_grids(shape, cell), dev)
    assert bool((grids != 0).any())
    return (("affine", lambda x, r, i, b, f, flags: warp.raw(lib, x, r, None, i, b, f, flags)),
            ("elastic", lambda x, r, i, b, f, flags: elastic.raw(lib, x, r, grids, cell, None, i, b, f, flags)))


@pytest.mark.parametrize("shape", WARP_SHAPES, ids=te.ids(WARP_SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_warps_copy_ragged_pack_blocks(dev, lib, dtype, shape):
    """A NaN row and an infinite row beside a finite one: the two tiles that are left are the output rule on their stored elements --
    their own bytes where nothing converts --, in both layouts and through both calls; the finite row's tile is what it is alone."""
    x = tiles_of(dtype, shape)
    xd, rows = x.to(dev), rows_t(te.LEFT_ROWS, dev)
    assert shape[1] % 4 == 0 and shape[1] % 32 != 0 and xd.data_ptr() % 16 == 0
    fill = fill_of(dtype)
    for name, call in warp_calls(lib, dev, shape):
        for flags in flag_sets(dtype):
            want = exact_output(wn.input_values(x[:2]), x, flags).to(dev)
            for interpolation, border in ((BILINEAR, MIRROR), (NEAREST, CONSTANT)):
                got = call(xd, rows, interpolation, border, fill, flags)
                assert got.dtype == want.dtype and torch.equal(got[:2], want), (name, flags, interpolation, border)
                if flags == 0:
                    assert torch.equal(bits(got[:2]), bits(xd[:2])), (name, "bytes")
                assert torch.equal(call(nhwc(xd), rows, interpolation, border, fill, flags | CL).permute(0, 3, 1, 2), got), (name, flags, "NHWC")
                assert torch.equal(call(off_by_one(xd), rows, interpolation, border, fill, flags), got), (name, flags, "one element off")
                assert not torch.equal(got[2], exact_output(wn.input_values(x[2]), x, flags).to(dev)), (name, flags, "the finite row moves its tile")
                if name == "affine":      # (the elastic call would want the tile's own grid alone)
                    assert torch.equal(call(xd[2:3].contiguous(), rows[2:3].contiguous(), interpolation, border, fill, flags), got[2:3]), (flags, "the finite row's tile alone")
        if dtype != torch.uint8:      # float tiles keep their bytes: NaN payloads, -0.0, infinities, a denormal
            special = te.with_specials(x).to(dev)
            for layout in ("nchw", "nhwc"):
                given, extra = (special, 0) if layout == "nchw" else (nhwc(special), CL)
                got = call(given, rows, BILINEAR, MIRROR, fill, extra)
                assert torch.equal(bits(got[:2]), bits(given[:2])), (name, layout, "special values")


@pytest.mark.parametrize("shape", WARP_SHAPES, ids=te.ids(WARP_SHAPES))
def test_mask_warps_copy_ragged_pack_blocks(dev, lib, shape):
    labels = (torch.arange(3 * shape[0] * shape[1]).reshape(3, *shape) * 37 % 256).to(torch.uint8).to(dev)
    rows = rows_t(te.LEFT_ROWS, dev)
    cell = 16
    grids = elastic.grids_t(en.test_grids(shape, cell), dev)
    for border, fill in ((CONSTANT, 0), (CONSTANT, 255), (MIRROR, 0)):
        for name, call in (("affine", lambda m: warp.raw_mask(lib, m, rows, None, border, fill)), ("elastic", lambda m: elastic.raw_mask(lib, m, rows, grids, cell, None, border, fill))):
            got = call(labels)
            assert torch.equal(got[:2], labels[:2]) and not torch.equal(got[2], labels[2]), (name, border, fill)
            assert torch.equal(call(off_by_one(labels)), got), (name, border, fill, "one byte off")
