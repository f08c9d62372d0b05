"""The affine warp on the GPU, through the C ABI (sx_affine_warp, sx_affine_warp_mask) and through ``affine_warp`` / ``affine_warp_mask``
/ ``affine_rows`` / ``AffineAugment``.

The yardstick is tests/_warp_numpy.py: the rule in float64 on the float32 values the kernel reads.  Float tiles hold values in [0, 1].
Batches are three tiles with three different rows in ONE launch.  The band of the bilinear comparison is DERIVED from the row and the
shape (``band_of``), not tuned: a float32 coordinate is off by at most ``2^-23 S``, S the sum of the absolute values of its three terms
at the far corner of the output tile, and the value moves by at most the largest difference of neighbours (255 levels, 1 on [0, 1]) times
that, per axis:
  uint8 output           0.5 + 255 * 2^-23 * (Sx + Sy) + 1e-3 levels (the half of rounding to nearest; 1e-3 covers the three float32 steps)
  float32 / float64      2^-23 * (Sx + Sy) + 1e-6 on [0, 1]
  float16 / bfloat16     plus 2^-12 / 2^-9: the rounding to the type
Everything else is exact: copies, integer shifts, flips and quarter turns, NaN / infinite rows, rows past the coordinate limit, the
output variants against the level result, nearest on rows whose coordinates are exact in float32, masks.

The tiles -- 1x1, 1x7, 2x2, 5x3 (axes of length 1 and 2, folds that run several times), 33x31 (odd width, a ragged block), 64x64, 65x130
(more than one block per axis, a ragged edge), 144x128 (packs), and the outputs 17x40 and 40x40 from 33x31, 24x24 from 64x64 (smaller and
larger than the source) -- are tests/test_blur_gpu.py's, shared."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import AffineAugment, _native, affine_rows, affine_warp, affine_warp_mask
from tests import _warp_numpy as wn
from tests.test_blur_gpu import CL, DTYPE_IDS, DTYPES, HALF_ULP_AT_1, OUT_FLAG, UNIT, nhwc, out_dtype_of, tiles_of
from tests.test_hsv_gpu import graph_nodes, off_by_one

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
NEAREST, BILINEAR = _native.WARP_INTERPOLATIONS["nearest"], _native.WARP_INTERPOLATIONS["bilinear"]
MIRROR, CONSTANT = _native.WARP_BORDERS["mirror"], _native.WARP_BORDERS["constant"]
BORDER_NAMES = {MIRROR: "mirror", CONSTANT: "constant"}
SHAPES = ((1, 1), (1, 7), (2, 2), (5, 3), (33, 31), (64, 64), (65, 130), (144, 128))
CASES = tuple((s, s) for s in SHAPES) + (((33, 31), (17, 40)), ((33, 31), (40, 40)), ((64, 64), (24, 24)))
CASE_IDS = [f"{s[0]}x{s[1]}" + (f"_to_{o[0]}x{o[1]}" if o != s else "") for s, o in CASES]
NAN_ROW = (NAN,) * 6
DYADIC_ROWS = ((0.75, -0.5, 3.0625, 0.5, 0.75, -2.1875), (1.0, 0.0, 0.25, 0.0, 1.0, -1.75), (0.5, 0.0, 0.5, 0.0, 0.5, 0.5))      # (exact in float32; the last: all ties)


def fill_of(dtype: torch.dtype) -> float:
    return 37.0 if dtype == torch.uint8 else 0.25


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ rows, calls and references
def as_rows(rows) -> tuple:
    """Rows as tuples of the float32 values' Python floats (hashable: the references are cached by them)."""
    return tuple(tuple(float(v) for v in np.asarray(r, dtype=np.float32)) for r in rows)


@lru_cache(maxsize=None)
def row_sets(shape: tuple, out: tuple) -> tuple:
    """Triples of rows for a case: rotations with scale, shear and sub-pixel shifts; a quarter-pixel shift, a translation several tile
    widths outside and a row that leaves its tile."""
    h, w = shape
    turned = as_rows(wn.rows64(3, shape, out, angle=(33.0, 45.0, -120.0), scale=(1.0, 0.7, 1.9), shear=(0.0, 8.0, -3.0), translate=((0.3, -1.7, 0.4), (-0.6, 2.2, 0.1))))
    other = as_rows([(1.0, 0.0, 0.25, 0.0, 1.0, 0.25), (1.0, 0.0, 3.25 * w + 0.4, 0.0, 1.0, -4.5 * h - 0.3)]) + (NAN_ROW,)
    return turned, other


def rows_t(rows, dev) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 6)


def raw(lib, x: torch.Tensor, rows: torch.Tensor, size=None, interpolation: int = BILINEAR, border: int = MIRROR, fill: float = 0.0, flags: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_affine_warp on the current stream; ``rows``: (R, 6) float32 on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    oh, ow = size or (h, w)
    if out is None:
        out = torch.empty((n, oh, ow, 3) if flags & CL else (n, 3, oh, ow), dtype=out_dtype_of(x, flags), device=x.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2 and x.is_contiguous()
    rc = lib.sx_affine_warp(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, oh, ow, rows.data_ptr(), rows.shape[0], interpolation, border, fill, flags,
                            _native.stream_ptr(x.device))
    assert rc == 0, _native.last_error(lib)
    return out


def raw_mask(lib, m: torch.Tensor, rows: torch.Tensor, size=None, border: int = CONSTANT, fill: int = 0) -> torch.Tensor:
    n, h, w = m.shape
    oh, ow = size or (h, w)
    out = torch.empty((n, oh, ow), dtype=torch.uint8, device=m.device)
    assert m.dtype == torch.uint8 and m.is_contiguous()
    rc = lib.sx_affine_warp_mask(m.data_ptr(), out.data_ptr(), n, h, w, oh, ow, rows.data_ptr(), rows.shape[0], border, fill, _native.stream_ptr(m.device))
    assert rc == 0, _native.last_error(lib)
    return out


@lru_cache(maxsize=None)
def reference(dtype: torch.dtype, shape: tuple, out: tuple, tile: int, row: tuple, interpolation: str, border: str) -> np.ndarray:
    """(3, OH, OW) float64: tile ``tile`` of ``tiles_of`` under ``row``, before the output rule."""
    got = wn.warp64(wn.input_values(tiles_of(dtype, shape)[tile]), row, out, interpolation=interpolation, border=border, fill=fill_of(dtype))
    got.setflags(write=False)
    return got


def reference_rows(dtype, shape, out, rows, interpolation="bilinear", border="mirror") -> np.ndarray:
    return np.stack([reference(dtype, shape, out, t, row, interpolation, border) for t, row in enumerate(rows)])


def band_of(row, shape, out, dtype: torch.dtype) -> float:
    """The derived band of a tile: levels for uint8 tiles, [0, 1] for float tiles."""
    s_x, s_y = wn.coordinate_slack(wn.effective_row(row, *shape, *out), *out)
    slack = 2.0**-23 * (s_x + s_y)
    return 0.5 + 255.0 * slack + 1e-3 if dtype == torch.uint8 else slack + 1e-6 + HALF_ULP_AT_1[dtype]


def check(got: torch.Tensor, want: np.ndarray, rows, shape, out, dtype, what) -> float:
    """``got``: (3, 3, OH, OW) on the CPU, levels or values; prints each tile's figure, then asserts."""
    worst = 0.0
    for t, row in enumerate(rows):
        err = float(np.abs(got[t].to(torch.float64).numpy() - want[t]).max())
        band = band_of(row, shape, out, dtype)
        print(f"{what}, tile {t}: max |out - float64| = {err:.3e} (band {band:.3e}, {err / band:.2f} of it)")
        assert err <= band, (what, t, err, band)
        worst = max(worst, err)
    return worst


def exact_output(value: np.ndarray, x: torch.Tensor, flags: int = 0) -> torch.Tensor:
    """The output rule on values that are stored elements or ``fill``."""
    return wn.to_output(value, x.dtype, out_dtype_of(x, flags), bool(flags & UNIT))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------ bilinear against the float64 restatement
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_bilinear_against_float64(dev, lib, dtype, case):
    shape, out = case
    x = tiles_of(dtype, shape)
    xd, xl = x.to(dev), nhwc(x).to(dev)
    fill = fill_of(dtype)
    for rows in row_sets(shape, out):
        r = rows_t(rows, dev)
        for border in (MIRROR, CONSTANT):
            want = reference_rows(dtype, shape, out, rows, "bilinear", BORDER_NAMES[border])
            got = raw(lib, xd, r, out, BILINEAR, border, fill)
            assert got.dtype == dtype and tuple(got.shape) == (3, 3, *out)
            check(got.cpu(), want, rows, shape, out, dtype, f"{DTYPE_IDS[DTYPES.index(dtype)]} {shape}->{out} {BORDER_NAMES[border]}")
            assert torch.equal(raw(lib, xl, r, out, BILINEAR, border, fill, CL).permute(0, 3, 1, 2), got), (rows, border, "NHWC")      # NCHW and NHWC: the same bits
            for t in range(3):      # a tile alone gives the bits it has inside the batch
                assert torch.equal(raw(lib, xd[t:t + 1].contiguous(), r[t:t + 1].contiguous(), out, BILINEAR, border, fill), got[t:t + 1]), (rows, border, t)
    # one row for the batch
    one = rows_t(row_sets(shape, out)[0][1:2], dev)
    assert torch.equal(raw(lib, xd, one, out), raw(lib, xd, one.repeat(3, 1), out))


@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[7], CASES[9]], ids=[CASE_IDS[4], CASE_IDS[6], CASE_IDS[7], CASE_IDS[9]])
@pytest.mark.parametrize("flags", [OUT_FLAG[torch.bfloat16], OUT_FLAG[torch.float16], UNIT, UNIT | OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16]],
                         ids=["bf16", "f16", "unit_f32", "unit_bf16", "unit_f16"])
def test_uint8_tiles_float_outputs_are_the_output_rule_on_the_level(dev, lib, flags, case):
    shape, out = case
    xd = tiles_of(torch.uint8, shape).to(dev)
    for rows in row_sets(shape, out):
        for interpolation, border in ((BILINEAR, MIRROR), (BILINEAR, CONSTANT), (NEAREST, CONSTANT)):
            r = rows_t(rows, dev)
            got = raw(lib, xd, r, out, interpolation, border, 37.0, flags)
            assert got.dtype == out_dtype_of(xd, flags)
            level = raw(lib, xd, r, out, interpolation, border, 37.0).cpu().to(torch.float32)      # the rounded 8-bit level of the plain call
            assert torch.equal(got.cpu(), ((level / 255.0) if flags & UNIT else level).to(got.dtype)), (flags, rows, interpolation, border)
            assert torch.equal(raw(lib, nhwc(xd), r, out, interpolation, border, 37.0, flags | CL).permute(0, 3, 1, 2), got)


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
def test_normalize_0_1_divides_a_float_tile_by_255(dev, lib, dtype):
    """The value rounded to the tile's type, divided by 255 in float32 (float64 tiles: in float64), rounded to the type again: an exact
    relation to the call without the flag, copies and fills included."""
    shape, out = (33, 31), (40, 40)
    xd = (tiles_of(dtype, shape).to(torch.float32) * 255.0).to(dtype).to(dev)      # (levels: what the flag is for)
    for rows in row_sets(shape, out):
        for interpolation in (BILINEAR, NEAREST):
            r = rows_t(rows, dev)
            value, unit = raw(lib, xd, r, out, interpolation, CONSTANT, 37.0).cpu(), raw(lib, xd, r, out, interpolation, CONSTANT, 37.0, UNIT).cpu()
            want = value / 255.0 if dtype == torch.float64 else (value.to(torch.float32) / 255.0).to(dtype)
            assert torch.equal(unit, want), (dtype, rows, interpolation)


# ------------------------------------------------------------------ exact, no tolerance
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_that_leave_the_tile_copy_crop_or_pad(dev, lib, dtype, case):
    """NaN / infinite rows: the anchor row -- the copy path where the sizes are equal, the centre crop or the centre pad otherwise."""
    shape, out = case
    x = tiles_of(dtype, shape)
    xd = x.to(dev)
    rows = (NAN_ROW, (1.0, 0.0, INF, 0.0, 1.0, 0.0), (0.3, 7.0, 1.0, -INF, 2.0, 5.0))
    anchor = wn.anchor_row(*shape, *out)
    for interpolation in (BILINEAR, NEAREST):
        for border in (MIRROR, CONSTANT):
            got = raw(lib, xd, rows_t(rows, dev), out, interpolation, border, fill_of(dtype))
            want = np.stack([wn.nearest(wn.input_values(x[t]), anchor, out, border=BORDER_NAMES[border], fill=fill_of(dtype)) for t in range(3)])
            assert torch.equal(got.cpu(), exact_output(want, x)), (dtype, case, interpolation, border)
            assert torch.equal(raw(lib, nhwc(xd), rows_t(rows, dev), out, interpolation, border, fill_of(dtype), CL).permute(0, 3, 1, 2), got)
    if shape == out:
        assert torch.equal(bits(got), bits(xd))      # the copy: the input's bits
    elif out[0] <= shape[0] and out[1] <= shape[1]:
        top, left = (shape[0] - out[0]) // 2, (shape[1] - out[1]) // 2
        assert torch.equal(got, xd[:, :, top:top + out[0], left:left + out[1]])      # the centre crop


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_integer_shifts_move_stored_elements(dev, lib, dtype):
    for shape, out in (((5, 3), (5, 3)), ((33, 31), (40, 40)), ((65, 130), (65, 130))):
        x = tiles_of(dtype, shape)
        rows = ((1.0, 0.0, 2.0, 0.0, 1.0, -3.0), (1.0, 0.0, -40.0, 0.0, 1.0, 7.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
        for border in (MIRROR, CONSTANT):
            want = np.stack([wn.nearest(wn.input_values(x[t]), rows[t], out, border=BORDER_NAMES[border], fill=fill_of(dtype)) for t in range(3)])
            for interpolation in (BILINEAR, NEAREST):      # (bilinear: fx = fy = 0 everywhere -- the stored element, no arithmetic)
                got = raw(lib, x.to(dev), rows_t(rows, dev), out, interpolation, border, fill_of(dtype))
                assert torch.equal(got.cpu(), exact_output(want, x)), (dtype, shape, out, border, interpolation)
        if shape == out:
            assert torch.equal(got[2], x[2].to(dev))


def special_floats(side: int) -> torch.Tensor:
    """(3, 3, side, side) float32 holding NaN payloads, -0.0, infinities and a denormal among ordinary values."""
    patterns = torch.tensor([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = tiles_of(torch.float32, (side, side)).clone().reshape(-1)
    x[::5] = patterns.repeat(x[::5].numel() // 7 + 1)[:x[::5].numel()]
    return x.reshape(3, 3, side, side)


@pytest.mark.parametrize("side", [2, 64], ids=["2x2", "64x64"])
def test_flips_and_quarter_turns_of_square_tiles_are_pixel_permutations(dev, lib, side):
    x = special_floats(side).to(dev)
    u8 = tiles_of(torch.uint8, (side, side)).to(dev)
    for turn in range(4):
        for flip in (False, True):
            rows = affine_rows(3, (side, side), angle=90.0 * turn, flip=flip, device=dev)
            for t, tile in ((x, x), (u8, u8)):
                want = torch.rot90(torch.flip(tile, (-1,)) if flip else tile, turn, (-2, -1))
                for interpolation in (BILINEAR, NEAREST):
                    for border in (MIRROR, CONSTANT):
                        got = raw(lib, tile, rows, None, interpolation, border, 0.5)
                        assert torch.equal(bits(got), bits(want)), (side, turn, flip, interpolation, border, tile.dtype)
            # a warp followed by its inverse: the flip is its own inverse and comes first, so undo the turn, then the flip
            back = raw(lib, raw(lib, x, rows), affine_rows(3, (side, side), angle=-90.0 * turn, device=dev))
            back = raw(lib, back, affine_rows(3, (side, side), flip=flip, device=dev))
            assert torch.equal(bits(back), bits(x)), (side, turn, flip)
    half = x.to(torch.float16)
    assert torch.equal(bits(raw(lib, half, affine_rows(3, (side, side), angle=90.0, device=dev))), bits(torch.rot90(half, 1, (-2, -1))))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_past_the_coordinate_limit_give_fill_everywhere(dev, lib, dtype):
    """A defined result of a valid input: every coordinate fails the float32 test before any integer is formed (the index path was read
    and tools/warp_index_check.cpp sweeps these rows on the host)."""
    limit = np.float32(wn.MAX_COORD)
    above = float(np.nextafter(limit, np.float32(np.inf)))
    for shape, out in (((5, 3), (5, 3)), ((33, 31), (40, 40)), ((65, 130), (65, 130))):
        x = tiles_of(dtype, shape)
        for rows in (((1.0, 0.0, 1e30, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -1e30), (3e38, 3e38, 3e38, 0.0, 1.0, 0.0)),
                     ((1.0, 0.0, above, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -above - 256.0), (0.0, 0.0, -3e38, 0.0, 0.0, 3e38))):
            for interpolation in (BILINEAR, NEAREST):
                for border in (MIRROR, CONSTANT):
                    got = raw(lib, x.to(dev), rows_t(rows, dev), out, interpolation, border, fill_of(dtype))
                    want = exact_output(np.full((3, 3, *out), fill_of(dtype)), x)
                    assert torch.equal(got.cpu(), want), (dtype, shape, rows, interpolation, border)
    # at the limit itself the pixel is inside it: column 0 sits at 2^22 - 3, folded into the tile -- a stored element, not the fill
    x = tiles_of(dtype, (5, 3))
    got = raw(lib, x.to(dev), rows_t(((1.0, 0.0, float(limit) - 3.0, 0.0, 1.0, 0.0),), dev), None, BILINEAR, MIRROR, fill_of(dtype)).cpu()
    want = wn.nearest(wn.input_values(x), (1.0, 0.0, float(limit) - 3.0, 0.0, 1.0, 0.0), border="mirror")
    assert torch.equal(got, exact_output(want, x))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_pointers_one_element_off_give_the_aligned_bits(dev, lib, dtype):
    shape = (144, 128)
    x = tiles_of(dtype, shape).to(dev)
    for rows in row_sets(shape, shape):
        r = rows_t(rows, dev)
        want = raw(lib, x, r)
        assert torch.equal(raw(lib, off_by_one(x), r), want)
        assert torch.equal(raw(lib, x, r, out=off_by_one(torch.empty_like(want))), want)
        assert torch.equal(raw(lib, off_by_one(nhwc(x)), r, flags=CL).permute(0, 3, 1, 2), want)
        assert torch.equal(raw(lib, x, off_by_one(r)), want)


# ------------------------------------------------------------------ nearest
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nearest_on_dyadic_rows_is_the_restatement(dev, lib, dtype, case):
    shape, out = case
    x = tiles_of(dtype, shape)
    for border in (MIRROR, CONSTANT):
        want = np.stack([wn.nearest(wn.input_values(x[t]), DYADIC_ROWS[t], out, border=BORDER_NAMES[border], fill=fill_of(dtype)) for t in range(3)])
        got = raw(lib, x.to(dev), rows_t(DYADIC_ROWS, dev), out, NEAREST, border, fill_of(dtype))
        assert torch.equal(got.cpu(), exact_output(want, x)), (dtype, case, border)
        assert torch.equal(raw(lib, nhwc(x).to(dev), rows_t(DYADIC_ROWS, dev), out, NEAREST, border, fill_of(dtype), CL).permute(0, 3, 1, 2), got)


@pytest.mark.parametrize("case", CASES[4:], ids=CASE_IDS[4:])
def test_nearest_on_generic_rows_away_from_half_integers(dev, lib, case):
    """Equal on every pixel whose float64 coordinates are further than 2^-23 S from a half-integer; a case may leave out at most 0.5 % of
    its pixels (printed; the restatement alone leaves out at most a handful)."""
    shape, out = case
    h, w = shape
    x = tiles_of(torch.uint8, shape)
    generic = as_rows(wn.rows64(3, shape, out, angle=(33.0, 45.0, 0.0), scale=(1.0, 0.7, 1.9), shear=(0.0, 8.0, 0.0), translate=((0.3, -1.7, 0.37), (-0.6, 2.2, 0.13))))
    far = as_rows([(1.0, 0.0, 3.25 * w + 0.4, 0.0, 1.0, -4.5 * h - 0.3), (1.0, 0.0, 0.37, 0.0, 1.0, -0.81), (0.9, 0.1, -7.31, -0.1, 0.9, 11.73)])
    for rows in (generic, far):
        for border in (MIRROR, CONSTANT):
            got = raw(lib, x.to(dev), rows_t(rows, dev), out, NEAREST, border, 37.0).cpu()
            for t, row in enumerate(rows):
                want = torch.from_numpy(wn.nearest(x[t].numpy(), row, out, border=BORDER_NAMES[border], fill=37).astype(np.uint8))
                sx, sy = wn.coords(row, *out)
                s_x, s_y = wn.coordinate_slack(row, *out)
                sure = (np.abs(sx - np.floor(sx) - 0.5) > 2.0**-23 * s_x) & (np.abs(sy - np.floor(sy) - 0.5) > 2.0**-23 * s_y)
                left_out = int((~sure).sum())
                print(f"nearest {shape}->{out} {BORDER_NAMES[border]} tile {t}: {left_out} of {sure.size} pixels within 2^-23 S of a half-integer")
                assert left_out <= 0.005 * sure.size, (case, row, left_out)
                keep = torch.from_numpy(sure).expand(3, -1, -1)
                assert torch.equal(got[t][keep], want[keep]), (case, border, t)


# ------------------------------------------------------------------ non-finite pixels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_a_nan_pixel_reaches_the_outputs_whose_taps_include_it(dev, lib, dtype):
    shape, place = (65, 130), (1, 31, 33)      # (channel, row, column): next to the block seams
    x = tiles_of(dtype, shape).clone()
    x[:, place[0], place[1], place[2]] = NAN
    seen = 0
    for rows in (row_sets(shape, shape)[0], as_rows([(1.0, 0.0, 0.0, 0.0, 1.0, 0.5), (1.0, 0.0, 0.5, 0.0, 1.0, 0.0), wn.IDENTITY])):
        for border in (MIRROR, CONSTANT):
            got = raw(lib, x.to(dev), rows_t(rows, dev), None, BILINEAR, border, 0.25).cpu()
            for t, row in enumerate(rows):
                want = wn.warp64(wn.input_values(x[t]), row, border=BORDER_NAMES[border], fill=0.25)
                expect = torch.from_numpy(np.isnan(want))
                assert not bool(expect[0].any()) and not bool(expect[2].any())      # (the other channels never see it)
                seen += int(expect.sum())
                assert torch.equal(torch.isnan(got[t]), expect), (dtype, row, border)
                err = float(np.abs(got[t].double().numpy() - want)[~expect.numpy()].max())
                assert err <= band_of(row, shape, shape, dtype), (dtype, row, err)
    assert seen >= 2 * (2 + 2 + 1), seen      # at least: a half-pixel shift puts it into two outputs, the identity into one, under both borders


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_mask_warp_is_the_nearest_image_warp_of_the_same_plane(dev, lib, case):
    shape, out = case
    labels = (torch.arange(3 * shape[0] * shape[1]).reshape(3, *shape) * 37 % 256).to(torch.uint8)      # every byte 0..255 where the plane is large enough
    image = labels.unsqueeze(1).expand(-1, 3, -1, -1).contiguous().to(dev)
    for rows in row_sets(shape, out) + (DYADIC_ROWS,):
        r = rows_t(rows, dev)
        for border, fill in ((CONSTANT, 0), (CONSTANT, 255), (MIRROR, 0)):
            got = raw_mask(lib, labels.to(dev), r, out, border, fill)
            assert torch.equal(got, raw(lib, image, r, out, NEAREST, border, float(fill))[:, 0]), (case, rows, border, fill)
    for border, fill in ((CONSTANT, 9), (MIRROR, 0)):      # and the restatement itself, where the coordinates are exact
        want = np.stack([wn.nearest(labels[t].numpy(), DYADIC_ROWS[t], out, border=BORDER_NAMES[border], fill=fill) for t in range(3)])
        assert torch.equal(raw_mask(lib, labels.to(dev), rows_t(DYADIC_ROWS, dev), out, border, fill).cpu(), torch.from_numpy(want.astype(np.uint8)))
    assert torch.equal(raw_mask(lib, off_by_one(labels.to(dev)), r, out, MIRROR, 0), got)


def test_labels_survive_and_a_mask_stays_aligned_with_its_image(dev, lib):
    side = 64
    labels = (torch.arange(3 * side * side).reshape(3, side, side) % 256).to(torch.uint8).to(dev)
    turned = raw_mask(lib, labels, affine_rows(3, (side, side), angle=90.0, flip=True, device=dev))
    assert torch.equal(turned, torch.rot90(torch.flip(labels, (-1,)), 1, (-2, -1)))      # bytes moved as bytes: every label 0..255 is still there
    assert torch.equal(torch.bincount(turned.reshape(-1).long(), minlength=256), torch.bincount(labels.reshape(-1).long(), minlength=256))
    # a mask made from a channel BEFORE the warp equals the same rule applied AFTER it (nearest, fill 0 on both sides)
    for shape, out in (((65, 130), (65, 130)), ((64, 64), (24, 24)), ((33, 31), (40, 40))):
        x = tiles_of(torch.uint8, shape).to(dev)
        before = (x[:, 0] > 128).to(torch.uint8)
        for rows in row_sets(shape, out):
            r = rows_t(rows, dev)
            after = raw(lib, x, r, out, NEAREST, CONSTANT, 0.0)
            assert torch.equal(raw_mask(lib, before, r, out, CONSTANT, 0), (after[:, 0] > 128).to(torch.uint8)), (shape, out, rows)
            assert torch.equal(affine_warp_mask(before, r, size=out), (affine_warp(x, r, size=out, interpolation="nearest", border="constant")[:, 0] > 128).to(torch.uint8))
            as_bool = affine_warp_mask(before.bool().unsqueeze(1), r, size=out, border="mirror")
            assert as_bool.dtype == torch.bool and tuple(as_bool.shape) == (3, 1, *out) and torch.equal(as_bool[:, 0].to(torch.uint8), raw_mask(lib, before, r, out, MIRROR, 0))


# ------------------------------------------------------------------ the module and the functional forms
def test_module_and_functional_form(dev, lib):
    shape = (65, 130)
    x = tiles_of(torch.uint8, shape).to(dev)
    rows = rows_t(row_sets(shape, shape)[0], dev)
    want = raw(lib, x, rows)
    assert torch.equal(affine_warp(x, rows), want)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        affine_warp(x.cpu(), rows)
    aug = AffineAugment(normalize_to_0_1=False)
    assert torch.equal(aug(x, rows), want) and torch.equal(aug(x, rows.cpu()), want)
    assert torch.equal(AffineAugment()(x, rows), raw(lib, x, rows, flags=UNIT))      # normalize_to_0_1 defaults to True, as the sibling modules'
    assert torch.equal(affine_warp(x, rows, out_dtype=torch.bfloat16), raw(lib, x, rows, flags=OUT_FLAG[torch.bfloat16]))
    assert torch.equal(affine_warp(nhwc(x), rows, channel_axis=-1), nhwc(want))
    assert torch.equal(affine_warp(x, rows, interpolation="nearest", border="constant", fill=200), raw(lib, x, rows, None, NEAREST, CONSTANT, 200.0))
    # one row for the batch: (1, 6) and (6,)
    one = raw(lib, x, rows[1:2].contiguous())
    assert torch.equal(affine_warp(x, rows[1:2]), one) and torch.equal(affine_warp(x, rows[1]), one)
    # CHW in, CHW out
    single = aug(x[1], rows[1:2])
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, want[1])
    # size= crops: 40 x 48 out of 65 x 130, in the same launch
    crop_rows = affine_rows(3, shape, (40, 48), angle=torch.tensor([10.0, 45.0, 90.0]), device=dev)
    cropped = affine_warp(x, crop_rows, size=(40, 48))
    assert tuple(cropped.shape) == (3, 3, 40, 48) and torch.equal(cropped, raw(lib, x, crop_rows, (40, 48)))
    assert torch.equal(AffineAugment(size=(40, 48), normalize_to_0_1=False)(x, crop_rows), cropped)
    # p = 0: every row is NaN -- the input comes back exactly; with size=: its centre crop
    assert torch.equal(AffineAugment(p=0.0, normalize_to_0_1=False)(x), x)
    assert torch.equal(AffineAugment(p=0.0, size=(40, 48), normalize_to_0_1=False)(x), x[:, :, 12:52, 41:89])
    # the pair returned with mask=: two launches, the same rows
    mask = (x[:, 0] > 128)
    tiles, warped = AffineAugment(interpolation="nearest", border="constant", normalize_to_0_1=False)(x, rows, mask=mask)
    assert torch.equal(tiles, raw(lib, x, rows, None, NEAREST, CONSTANT, 0.0)) and warped.dtype == torch.bool and torch.equal(warped, tiles[:, 0] > 128)
    tiles, warped = aug(x, rows, mask=mask.to(torch.uint8).unsqueeze(1))
    assert torch.equal(tiles, want) and tuple(warped.shape) == (3, 1, *shape) and torch.equal(warped[:, 0], raw_mask(lib, mask.to(torch.uint8), rows, None, MIRROR, 0))
    tile, flat = aug(x[1], rows[1:2], mask=mask[1])
    assert torch.equal(tile, want[1]) and tuple(flat.shape) == shape
    # a draw: the rows sample_rows gives with the same seed, on the device when the generator is there
    for where in ("cpu", dev):
        make = lambda: AffineAugment((-30.0, 30.0), scale=(0.8, 1.25), translate=(0.1, 0.1), p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5))  # noqa: E731
        got = make()(x)
        again = make().sample_rows(3, shape, dev)
        assert torch.equal(got, raw(lib, x, again.contiguous()))
        left = torch.isnan(again).any(dim=1)
        assert torch.equal(got[left], x[left])
    basic = AffineAugment("quarter", normalize_to_0_1=False, generator=torch.Generator().manual_seed(1))      # the eight symmetries: pixel permutations of a square tile
    square = tiles_of(torch.uint8, (64, 64)).to(dev)
    turned = basic(square)
    assert torch.equal(turned.reshape(3, 3, -1).sort(dim=-1).values, square.reshape(3, 3, -1).sort(dim=-1).values)


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("with_mask", [False, True], ids=["tiles", "tiles_and_mask"])
def test_a_captured_forward_replays_with_new_rows_and_images(dev, with_mask):
    shape = (65, 130)
    first_x, second_x = tiles_of(torch.uint8, shape).to(dev), tiles_of(torch.uint8, shape).flip(0).contiguous().to(dev)
    first, second = rows_t(row_sets(shape, shape)[0], dev), rows_t(row_sets(shape, shape)[1], dev)
    aug = AffineAugment(normalize_to_0_1=False, size=(40, 48))
    mask_of = lambda t: (t[:, 0] > 128).to(torch.uint8)  # noqa: E731
    call = (lambda t, r, m: aug(t, r, mask=m)) if with_mask else (lambda t, r, m: (aug(t, r), None))
    want_first, want_second = call(first_x, first, mask_of(first_x)), call(second_x, second, mask_of(second_x))
    assert not torch.equal(want_first[0], want_second[0])
    x, buf, m = first_x.clone(), first.clone(), mask_of(first_x)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        call(x, buf, m)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call(x, buf, m)
        types, roots, edges = graph_nodes(dev)
    # kernel nodes only (hipGraphNodeTypeKernel = 0): ONE for the tiles, two with a mask, in a single branch; no memset node (2), no copy (1)
    assert types == ([0, 0] if with_mask else [0]), types
    assert roots == 1 and edges == (1 if with_mask else 0)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], want_first[0]) and (not with_mask or torch.equal(out[1], want_first[1]))
    buf.copy_(second)
    x.copy_(second_x)
    m.copy_(mask_of(second_x))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], want_second[0]) and (not with_mask or torch.equal(out[1], want_second[1]))


# ------------------------------------------------------------------ the C ABI's refusals leave the output alone
def test_argument_errors_launch_nothing(dev, lib):
    x = tiles_of(torch.uint8, (33, 31)).to(dev)
    out, mask_out = torch.full_like(x, 7), torch.full((3, 33, 31), 7, dtype=torch.uint8, device=dev)
    rows, mask = rows_t((wn.IDENTITY,) * 3, dev), torch.ones(3, 33, 31, dtype=torch.uint8, device=dev)
    code, stream, bad = _native.DTYPE_CODES[torch.uint8], _native.stream_ptr(dev), _native.SX_ERR_BAD_ARG
    p = lambda t: t.data_ptr()      # noqa: E731

    def warp(images=p(x), to=p(out), dtype=code, n=3, h=33, w=31, oh=33, ow=31, r=p(rows), n_rows=3, interpolation=BILINEAR, border=MIRROR, fill=0.0, flags=0):
        return lib.sx_affine_warp(images, to, dtype, n, h, w, oh, ow, r, n_rows, interpolation, border, fill, flags, stream)

    def warp_mask(m=p(mask), to=p(mask_out), n=3, h=33, w=31, oh=33, ow=31, r=p(rows), n_rows=3, border=CONSTANT, fill=0):
        return lib.sx_affine_warp_mask(m, to, n, h, w, oh, ow, r, n_rows, border, fill, stream)

    for kwargs, word in (({"images": None}, "null"), ({"to": None}, "null"), ({"r": None}, "null"), ({"h": -33}, "positive"), ({"n": -3}, "positive"), ({"oh": 0}, "positive"), ({"ow": -1}, "positive"),
                         ({"n_rows": 2}, "n_rows"), ({"interpolation": 2}, "interpolation"), ({"border": 2}, "border"), ({"fill": NAN}, "fill"), ({"fill": INF}, "fill"),
                         ({"flags": 1 << 20}, "flags"), ({"flags": OUT_FLAG[torch.bfloat16] | OUT_FLAG[torch.float16]}, "one of the two")):
        assert warp(**kwargs) == bad and word in _native.last_error(lib), kwargs
    assert warp(dtype=17) == _native.SX_ERR_DTYPE
    for kwargs, word in (({"m": None}, "null"), ({"to": None}, "null"), ({"r": None}, "null"), ({"w": 0}, "positive"), ({"oh": -2}, "positive"), ({"n_rows": 2}, "n_rows"), ({"border": -1}, "border"),
                         ({"fill": 256}, "0..255"), ({"fill": -1}, "0..255")):
        assert warp_mask(**kwargs) == bad and word in _native.last_error(lib), kwargs
    torch.cuda.synchronize(dev)
    assert bool((out == 7).all()) and bool((mask_out == 7).all())
