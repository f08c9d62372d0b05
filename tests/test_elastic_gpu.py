"""The elastic warp on the GPU, through the C ABI (sx_elastic_warp, sx_elastic_warp_mask) and through ``elastic_warp`` /
``elastic_warp_mask`` / ``elastic_grids`` / ``ElasticAugment``.

The yardstick is tests/_elastic_numpy.py: the rule in float64 on the float32 values the kernel reads, and the band DERIVED there from the
rule's operation count (``coordinate_band``, ``value_band``) -- tests/test_warp_gpu.py's band with a displacement term.  Batches are three
tiles with three different rows AND three different grids (control displacements of standard deviation 1, 2 and 3 pixels) in ONE launch.
The cells: 4 (the smallest: 11 control points per block and axis), 7 (does not divide the block's 32), 16, 64 (wider than a block) and 4096
(wider than the tile: GH = GW = 4); the row sets of tests/test_warp_gpu.py alternate over them.  Everything but the bilinear and the
nearest comparison is exact: a zero grid against sx_affine_warp, tiles that are left, displacements that are not finite, pointers one
element off, masks, the module against the functional form.  The tiles and outputs are tests/test_warp_gpu.py's."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import AffineAugment, ElasticAugment, _native, affine_rows, elastic_grid_shape, elastic_grids, elastic_warp, elastic_warp_mask
from tests import _elastic_numpy as en
from tests import _warp_numpy as wn
from tests.test_blur_gpu import CL, DTYPE_IDS, DTYPES, HALF_ULP_AT_1, OUT_FLAG, UNIT, nhwc, out_dtype_of, tiles_of
from tests.test_hsv_gpu import graph_nodes, off_by_one
from tests.test_warp_gpu import BILINEAR, BORDER_NAMES, CASE_IDS, CASES, CONSTANT, INF, MIRROR, NAN, NAN_ROW, NEAREST, as_rows, bits, exact_output, fill_of, row_sets, rows_t
from tests.test_warp_gpu import raw as raw_affine
from tests.test_warp_gpu import raw_mask as raw_affine_mask

pytestmark = pytest.mark.gpu

CELLS = (4, 7, 16, 64, 4096)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ grids, calls and references
@lru_cache(maxsize=None)
def grids_of(out: tuple, cell: int) -> np.ndarray:
    """(3, 2, GH, GW) float32: the case's three grids, standard deviations 1, 2 and 3 pixels."""
    g = en.test_grids(out, cell)
    g.setflags(write=False)
    return g


def grids_t(grids: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(grids, dtype=np.float32)).to(dev)      # (a copy: the cached grids are read-only)


def plan(shape: tuple, out: tuple):
    """(cell, rows, grids) of a case: every cell, the two row sets alternating."""
    for i, cell in enumerate(CELLS):
        yield cell, row_sets(shape, out)[i % 2], grids_of(out, cell)


def raw(lib, x: torch.Tensor, rows: torch.Tensor, grids: torch.Tensor, cell: int, size=None, interpolation: int = BILINEAR, border: int = MIRROR, fill: float = 0.0, flags: int = 0,
        out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_elastic_warp on the current stream; ``rows``: (R, 6), ``grids``: (G, 2, GH, GW) float32 on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    oh, ow = size or (h, w)
    if out is None:
        out = torch.empty((n, oh, ow, 3) if flags & CL else (n, 3, oh, ow), dtype=out_dtype_of(x, flags), device=x.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2 and x.is_contiguous()
    assert grids.dtype == torch.float32 and grids.is_contiguous() and tuple(grids.shape[1:]) == (2, *elastic_grid_shape((oh, ow), cell)) and grids.is_cuda
    rc = lib.sx_elastic_warp(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, oh, ow, rows.data_ptr(), rows.shape[0], grids.data_ptr(), grids.shape[0], cell, interpolation,
                             border, fill, flags, _native.stream_ptr(x.device))
    assert rc == 0, _native.last_error(lib)
    return out


def raw_mask(lib, m: torch.Tensor, rows: torch.Tensor, grids: torch.Tensor, cell: int, size=None, border: int = CONSTANT, fill: int = 0) -> torch.Tensor:
    n, h, w = m.shape
    oh, ow = size or (h, w)
    out = torch.empty((n, oh, ow), dtype=torch.uint8, device=m.device)
    assert m.dtype == torch.uint8 and m.is_contiguous() and grids.is_contiguous() and tuple(grids.shape[1:]) == (2, *elastic_grid_shape((oh, ow), cell)) and grids.is_cuda
    rc = lib.sx_elastic_warp_mask(m.data_ptr(), out.data_ptr(), n, h, w, oh, ow, rows.data_ptr(), rows.shape[0], grids.data_ptr(), grids.shape[0], cell, border, fill, _native.stream_ptr(m.device))
    assert rc == 0, _native.last_error(lib)
    return out


@lru_cache(maxsize=None)
def reference(dtype: torch.dtype, shape: tuple, out: tuple, tile: int, row: tuple, cell: int, border: str) -> np.ndarray:
    """(3, OH, OW) float64: tile ``tile`` of ``tiles_of`` under ``row`` and grid ``tile`` of the case, bilinear, before the output rule."""
    got = en.warp64(wn.input_values(tiles_of(dtype, shape)[tile]), row, grids_of(out, cell)[tile], cell, out, border=border, fill=fill_of(dtype))
    got.setflags(write=False)
    return got


def band_of(row, grid, shape, out, dtype: torch.dtype) -> float:
    return en.value_band(wn.effective_row(row, *shape, *out), grid if np.isfinite(np.asarray(row, dtype=np.float32)).all() else np.zeros_like(grid), out, dtype == torch.uint8, HALF_ULP_AT_1.get(dtype, 0.0))


# ------------------------------------------------------------------ bilinear against the float64 restatement
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_bilinear_against_float64(dev, lib, dtype, case):
    shape, out = case
    x = tiles_of(dtype, shape)
    xd, xl = x.to(dev), nhwc(x).to(dev)
    fill = fill_of(dtype)
    for cell, rows, grids in plan(shape, out):
        r, g = rows_t(rows, dev), grids_t(grids, dev)
        for border in (MIRROR, CONSTANT):
            got = raw(lib, xd, r, g, cell, out, BILINEAR, border, fill)
            assert got.dtype == dtype and tuple(got.shape) == (3, 3, *out)
            host = got.cpu()
            for t, row in enumerate(rows):
                want = reference(dtype, shape, out, t, row, cell, BORDER_NAMES[border])
                err, band = float(np.abs(host[t].to(torch.float64).numpy() - want).max()), band_of(row, grids[t], shape, out, dtype)
                print(f"{DTYPE_IDS[DTYPES.index(dtype)]} {shape}->{out} cell {cell} {BORDER_NAMES[border]}, tile {t}: max |out - float64| = {err:.3e} (band {band:.3e}, {err / band:.2f} of it)")
                assert err <= band, (dtype, case, cell, border, t, err, band)
            assert torch.equal(raw(lib, xl, r, g, cell, out, BILINEAR, border, fill, CL).permute(0, 3, 1, 2), got), (cell, border, "NHWC")      # NCHW and NHWC: the same bits
            for t in range(3):      # a tile alone gives the bits it has inside the batch
                assert torch.equal(raw(lib, xd[t:t + 1].contiguous(), r[t:t + 1].contiguous(), g[t:t + 1].contiguous(), cell, out, BILINEAR, border, fill), got[t:t + 1]), (cell, border, t)
        # one grid for the batch is N equal grids; and one row for the batch with it
        one = g[1:2].contiguous()
        assert torch.equal(raw(lib, xd, r, one, cell, out), raw(lib, xd, r, one.repeat(3, 1, 1, 1), cell, out)), cell
        assert torch.equal(raw(lib, xd, r[:1].contiguous(), one, cell, out), raw(lib, xd, r[:1].repeat(3, 1), one.repeat(3, 1, 1, 1), cell, out)), cell


# ------------------------------------------------------------------ exact, no tolerance
def variants_of(dtype: torch.dtype) -> tuple:
    if dtype == torch.uint8:
        return (0, OUT_FLAG[torch.bfloat16], OUT_FLAG[torch.float16], UNIT, UNIT | OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16])
    return (0, UNIT)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_zero_grid_is_the_affine_warp_bit_for_bit(dev, lib, case):
    """Every case, cell, element type and output variant, both interpolations, both borders, both layouts: the weights are >= 0, every
    product and sum of the two passes is a zero, and s + 0.0 keeps the taps and the fractions."""
    shape, out = case
    for dtype in DTYPES:
        x = tiles_of(dtype, shape).to(dev)
        for cell, rows, grids in plan(shape, out):
            r, zero = rows_t(rows, dev), torch.zeros((3, *grids.shape[1:]), dtype=torch.float32, device=dev)
            for flags in variants_of(dtype):
                for interpolation in (BILINEAR, NEAREST):
                    for border in (MIRROR, CONSTANT):
                        want = raw_affine(lib, x, r, out, interpolation, border, fill_of(dtype), flags)
                        assert torch.equal(bits(raw(lib, x, r, zero, cell, out, interpolation, border, fill_of(dtype), flags)), bits(want)), (dtype, case, cell, flags, interpolation, border)
            assert torch.equal(bits(raw(lib, x, r, zero[:1].contiguous(), cell, out)), bits(raw_affine(lib, x, r, out)))
            assert torch.equal(raw(lib, nhwc(x), r, -zero, cell, out, flags=CL), raw_affine(lib, nhwc(x), r, out, flags=CL))      # (a grid of -0.0 as well)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_that_leave_the_tile_copy_crop_or_pad_whatever_the_grid(dev, lib, dtype, case):
    """NaN / infinite rows with a garbage grid: sx_affine_warp's result -- the copy path where the sizes are equal, the centre crop or the
    centre pad otherwise; the grid is not read."""
    shape, out = case
    x = tiles_of(dtype, shape)
    xd = x.to(dev)
    rows = rows_t((NAN_ROW, (1.0, 0.0, INF, 0.0, 1.0, 0.0), (0.3, 7.0, 1.0, -INF, 2.0, 5.0)), dev)
    anchor = wn.anchor_row(*shape, *out)
    for cell in CELLS:
        garbage = grids_t(grids_of(out, cell), dev).clone() * 1e3
        garbage.view(-1)[::3] = NAN
        garbage.view(-1)[1::7] = 1e30
        for interpolation in (BILINEAR, NEAREST):
            for border in (MIRROR, CONSTANT):
                got = raw(lib, xd, rows, garbage, cell, out, interpolation, border, fill_of(dtype))
                want = np.stack([wn.nearest(wn.input_values(x[t]), anchor, out, border=BORDER_NAMES[border], fill=fill_of(dtype)) for t in range(3)])
                assert torch.equal(got.cpu(), exact_output(want, x)), (dtype, case, cell, interpolation, border)
                assert torch.equal(bits(got), bits(raw_affine(lib, xd, rows, out, interpolation, border, fill_of(dtype))))
                assert torch.equal(raw(lib, nhwc(xd), rows, garbage, cell, out, interpolation, border, fill_of(dtype), CL).permute(0, 3, 1, 2), got)
        if shape == out:
            assert torch.equal(bits(got), bits(xd))      # the copy: the input's bits


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_displacements_that_are_not_finite_or_huge_give_fill_everywhere(dev, lib, dtype):
    """A defined result of a valid input: the coordinate fails the float32 limit test before any integer is formed
    (tools/elastic_index_check.cpp sweeps these grids on the host)."""
    for shape, out in (((5, 3), (5, 3)), ((33, 31), (40, 40)), ((65, 130), (65, 130))):
        x = tiles_of(dtype, shape)
        rows = rows_t(row_sets(shape, out)[0], dev)
        for cell in CELLS:
            gh, gw = elastic_grid_shape(out, cell)
            for values in ((NAN, INF, 1e30), (-INF, -1e30, NAN)):
                grids = torch.tensor(values, dtype=torch.float32, device=dev).view(3, 1, 1, 1).expand(3, 2, gh, gw).contiguous()
                for interpolation in (BILINEAR, NEAREST):
                    for border in (MIRROR, CONSTANT):
                        got = raw(lib, x.to(dev), rows, grids, cell, out, interpolation, border, fill_of(dtype))
                        assert torch.equal(got.cpu(), exact_output(np.full((3, 3, *out), fill_of(dtype)), x)), (dtype, shape, cell, values, interpolation, border)
    # one plane alone is enough: dy = NaN with dx = 0
    grids = torch.zeros((1, 2, *elastic_grid_shape((33, 31), 16)), dtype=torch.float32, device=dev)
    grids[:, 1] = NAN
    x = tiles_of(dtype, (33, 31))
    assert torch.equal(raw(lib, x.to(dev), rows_t((wn.IDENTITY,), dev), grids, 16, None, BILINEAR, MIRROR, fill_of(dtype)).cpu(), exact_output(np.full((3, 3, 33, 31), fill_of(dtype)), x))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_pointers_one_element_off_give_the_aligned_bits(dev, lib, dtype):
    shape = (144, 128)
    x = tiles_of(dtype, shape).to(dev)
    for cell, rows, grids in plan(shape, shape):
        r, g = rows_t(rows, dev), grids_t(grids, dev)
        want = raw(lib, x, r, g, cell)
        assert torch.equal(raw(lib, off_by_one(x), r, g, cell), want)
        assert torch.equal(raw(lib, x, r, g, cell, out=off_by_one(torch.empty_like(want))), want)
        assert torch.equal(raw(lib, off_by_one(nhwc(x)), r, g, cell, flags=CL).permute(0, 3, 1, 2), want)
        assert torch.equal(raw(lib, x, off_by_one(r), g, cell), want)
        assert torch.equal(raw(lib, x, r, off_by_one(g), cell), want)


# ------------------------------------------------------------------ nearest
@pytest.mark.parametrize("case", CASES[4:], ids=CASE_IDS[4:])
def test_nearest_away_from_half_integers_is_the_restatement(dev, lib, case):
    """Equal on every pixel whose float64 coordinates are further than the coordinate band from a half-integer; a tile may leave out at most
    1 % of its pixels (printed; tests/test_elastic_cpu.py holds the restatement alone to that cap)."""
    shape, out = case
    x = tiles_of(torch.uint8, shape)
    generic = as_rows(wn.rows64(3, shape, out, angle=(33.0, 45.0, 0.0), scale=(1.0, 0.7, 1.9), shear=(0.0, 8.0, 0.0), translate=((0.3, -1.7, 0.37), (-0.6, 2.2, 0.13))))
    for cell in CELLS:
        grids = grids_of(out, cell)
        for border in (MIRROR, CONSTANT):
            got = raw(lib, x.to(dev), rows_t(generic, dev), grids_t(grids, dev), cell, out, NEAREST, border, 37.0).cpu()
            for t, row in enumerate(generic):
                want = torch.from_numpy(en.warp64(x[t].numpy(), row, grids[t], cell, out, interpolation="nearest", border=BORDER_NAMES[border], fill=37).astype(np.uint8))
                sx, sy = en.coords(row, grids[t], out, cell)
                e_x, e_y = en.coordinate_band(row, grids[t], out)
                sure = (np.abs(sx - np.floor(sx) - 0.5) > e_x) & (np.abs(sy - np.floor(sy) - 0.5) > e_y)
                left_out = int((~sure).sum())
                print(f"nearest {shape}->{out} cell {cell} {BORDER_NAMES[border]} tile {t}: {left_out} of {sure.size} pixels within the band of a half-integer")
                assert left_out <= 0.01 * sure.size, (case, cell, row, left_out)
                keep = torch.from_numpy(sure).expand(3, -1, -1)
                assert torch.equal(got[t][keep], want[keep]), (case, cell, border, t)


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_mask_warp_is_the_nearest_image_warp_of_the_same_plane(dev, lib, case):
    shape, out = case
    labels = (torch.arange(3 * shape[0] * shape[1]).reshape(3, *shape) * 37 % 256).to(torch.uint8)      # every byte 0..255 where the plane is large enough
    image = labels.unsqueeze(1).expand(-1, 3, -1, -1).contiguous().to(dev)
    for cell, rows, grids in plan(shape, out):
        r, g = rows_t(rows, dev), grids_t(grids, dev)
        for border, fill in ((CONSTANT, 0), (CONSTANT, 255), (MIRROR, 0)):
            got = raw_mask(lib, labels.to(dev), r, g, cell, out, border, fill)
            assert torch.equal(got, raw(lib, image, r, g, cell, out, NEAREST, border, float(fill))[:, 0]), (case, cell, border, fill)
        assert torch.equal(raw_mask(lib, off_by_one(labels.to(dev)), r, g, cell, out, MIRROR, 0), got)
        assert torch.equal(raw_mask(lib, labels.to(dev), r, torch.zeros_like(g), cell, out, MIRROR, 0), raw_affine_mask(lib, labels.to(dev), r, out, MIRROR, 0))      # a zero grid: the affine mask warp


def test_labels_survive_and_a_mask_stays_aligned_with_its_image(dev, lib):
    side = 64
    labels = (torch.arange(3 * side * side).reshape(3, side, side) % 256).to(torch.uint8).to(dev)
    turn = affine_rows(3, (side, side), angle=90.0, flip=True, device=dev)
    # a displacement by whole pixels (a constant grid) on top of a quarter turn: bytes moved as bytes, every pixel inside the tile is a stored label
    shift = torch.zeros((1, 2, *elastic_grid_shape((side, side), 16)), dtype=torch.float32, device=dev)
    shift[:, 0], shift[:, 1] = 3.0, -2.0
    moved = raw_mask(lib, labels, turn, shift, 16, None, MIRROR, 0)
    shifted_rows = turn.clone()
    shifted_rows[:, 2] += 3.0
    shifted_rows[:, 5] -= 2.0
    assert torch.equal(moved, raw_affine_mask(lib, labels, shifted_rows, None, MIRROR, 0))
    warped = raw_mask(lib, labels, turn, grids_t(grids_of((side, side), 16), dev), 16, None, MIRROR, 0)
    assert set(warped.reshape(-1).tolist()) == set(range(256))      # labels 0..255 are all still there: nothing was interpolated or scaled
    # a mask made from a channel BEFORE the warp equals the same rule applied AFTER it (nearest, fill 0 on both sides)
    for shape, out in (((65, 130), (65, 130)), ((64, 64), (24, 24)), ((33, 31), (40, 40))):
        x = tiles_of(torch.uint8, shape).to(dev)
        before = (x[:, 0] > 128).to(torch.uint8)
        for cell, rows, grids in plan(shape, out):
            r, g = rows_t(rows, dev), grids_t(grids, dev)
            after = raw(lib, x, r, g, cell, out, NEAREST, CONSTANT, 0.0)
            assert torch.equal(raw_mask(lib, before, r, g, cell, out, CONSTANT, 0), (after[:, 0] > 128).to(torch.uint8)), (shape, out, cell)
            assert torch.equal(elastic_warp_mask(before, g, cell=cell, rows=r, size=out), (elastic_warp(x, g, cell=cell, rows=r, size=out, interpolation="nearest", border="constant")[:, 0] > 128).to(torch.uint8))
            as_bool = elastic_warp_mask(before.bool().unsqueeze(1), g, cell=cell, rows=r, size=out, border="mirror")
            assert as_bool.dtype == torch.bool and tuple(as_bool.shape) == (3, 1, *out) and torch.equal(as_bool[:, 0].to(torch.uint8), raw_mask(lib, before, r, g, cell, out, MIRROR, 0))


# ------------------------------------------------------------------ the module and the functional forms
def test_module_and_functional_form(dev, lib):
    shape, cell = (65, 130), 16
    x = tiles_of(torch.uint8, shape).to(dev)
    rows, grids = rows_t(row_sets(shape, shape)[0], dev), grids_t(grids_of(shape, cell), dev)
    want = raw(lib, x, rows, grids, cell)
    assert torch.equal(elastic_warp(x, grids, cell=cell, rows=rows), want)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        elastic_warp(x.cpu(), grids, cell=cell)
    anchor = rows_t((wn.IDENTITY,), dev)
    assert torch.equal(elastic_warp(x, grids, cell=cell), raw(lib, x, anchor, grids, cell))      # rows=None: the anchor row
    aug = ElasticAugment(cell=cell, normalize_to_0_1=False)
    assert torch.equal(aug(x, grids, rows), want) and torch.equal(aug(x, grids.cpu(), rows.cpu()), want)
    assert torch.equal(ElasticAugment(cell=cell)(x, grids, rows), raw(lib, x, rows, grids, cell, flags=UNIT))      # normalize_to_0_1 defaults to True, as the sibling modules'
    assert torch.equal(elastic_warp(x, grids, cell=cell, rows=rows, out_dtype=torch.bfloat16), raw(lib, x, rows, grids, cell, flags=OUT_FLAG[torch.bfloat16]))
    assert torch.equal(elastic_warp(nhwc(x), grids, cell=cell, rows=rows, channel_axis=-1), nhwc(want))
    assert torch.equal(elastic_warp(x, grids, cell=cell, rows=rows, interpolation="nearest", border="constant", fill=200), raw(lib, x, rows, grids, cell, None, NEAREST, CONSTANT, 200.0))
    # one grid for the batch: (1, 2, GH, GW) and (2, GH, GW)
    one = raw(lib, x, rows, grids[1:2].contiguous(), cell)
    assert torch.equal(elastic_warp(x, grids[1:2], cell=cell, rows=rows), one) and torch.equal(elastic_warp(x, grids[1], cell=cell, rows=rows), one)
    # CHW in, CHW out
    single = aug(x[1], grids[1], rows[1:2])
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, want[1])
    # size= crops: 40 x 48 out of 65 x 130, in the same launch; rows=None: the centre crop's row
    small = grids_t(grids_of((40, 48), cell), dev)
    crop_rows = affine_rows(3, shape, (40, 48), angle=torch.tensor([10.0, 45.0, 90.0]), device=dev)
    cropped = elastic_warp(x, small, cell=cell, rows=crop_rows, size=(40, 48))
    assert tuple(cropped.shape) == (3, 3, 40, 48) and torch.equal(cropped, raw(lib, x, crop_rows, small, cell, (40, 48)))
    assert torch.equal(elastic_warp(x, small, cell=cell, size=(40, 48)), raw(lib, x, rows_t((wn.anchor_row(*shape, 40, 48),), dev), small, cell, (40, 48)))
    assert torch.equal(elastic_warp(x, torch.zeros_like(small), cell=cell, size=(40, 48)), x[:, :, 12:52, 41:89])
    # the pair returned with mask=: two launches, the same rows and grids
    mask = (x[:, 0] > 128)
    tiles, warped = ElasticAugment(cell=cell, interpolation="nearest", border="constant", normalize_to_0_1=False)(x, grids, rows, mask=mask)
    assert torch.equal(tiles, raw(lib, x, rows, grids, cell, None, NEAREST, CONSTANT, 0.0)) and warped.dtype == torch.bool and torch.equal(warped, tiles[:, 0] > 128)
    tiles, warped = aug(x, grids, rows, mask=mask.to(torch.uint8).unsqueeze(1))
    assert torch.equal(tiles, want) and tuple(warped.shape) == (3, 1, *shape) and torch.equal(warped[:, 0], raw_mask(lib, mask.to(torch.uint8), rows, grids, cell, None, MIRROR, 0))
    tile, flat = aug(x[1], grids[1], rows[1:2], mask=mask[1])
    assert torch.equal(tile, want[1]) and tuple(flat.shape) == shape


def test_a_draw_is_the_functional_form_on_the_sampled_rows_and_grids(dev, lib):
    shape, size = (65, 130), (40, 48)
    x = tiles_of(torch.uint8, shape).to(dev)
    for where in ("cpu", dev):
        affine = lambda: AffineAugment((-30.0, 30.0), scale=(0.8, 1.25), translate=(0.1, 0.1), p=0.5, size=size, generator=torch.Generator(device=where).manual_seed(5))  # noqa: E731
        make = lambda **k: ElasticAugment((0.5, 3.0), 7, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(6), **k)  # noqa: E731
        for kwargs in ({"p": 0.5, "size": size}, {"affine": affine(), "p": 0.5}, {"affine": affine()}):
            got = make(**kwargs)(x)
            if "affine" in kwargs:
                kwargs = {**kwargs, "affine": affine()}
            rows, grids = make(**kwargs).sample(3, shape, dev)
            assert rows.device == dev and grids.device == dev and tuple(grids.shape) == (3, 2, *elastic_grid_shape(size, 7))
            assert torch.equal(got, elastic_warp(x, grids, cell=7, rows=rows, size=size)) and torch.equal(got, raw(lib, x, rows.contiguous(), grids.contiguous(), 7, size))
    # p = 0: every grid is zero -- the affine module's output on the same rows, bit for bit; without affine the input (its centre crop)
    for where in ("cpu", dev):
        affine = lambda: AffineAugment((-30.0, 30.0), scale=(0.8, 1.25), shear=(-5.0, 5.0), p=0.7, size=size, generator=torch.Generator(device=where).manual_seed(8))  # noqa: E731
        assert torch.equal(ElasticAugment((1.0, 3.0), 16, affine=affine(), p=0.0, generator=torch.Generator(device=where).manual_seed(1))(x), affine()(x))
    assert torch.equal(ElasticAugment(p=0.0, normalize_to_0_1=False)(x), x)
    assert torch.equal(ElasticAugment(p=0.0, size=size, normalize_to_0_1=False)(x), x[:, :, 12:52, 41:89])
    on_device = elastic_grids(3, size, 7, torch.tensor([0.0, 1.0, 2.0], device=dev), generator=torch.Generator(device=dev).manual_seed(4))
    assert on_device.device == dev and not bool(on_device[0].any()) and bool(on_device[1].any())


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("with_mask", [False, True], ids=["tiles", "tiles_and_mask"])
def test_a_captured_forward_replays_with_new_grids_rows_and_images(dev, with_mask):
    shape, size, cell = (65, 130), (40, 48), 16
    first_x, second_x = tiles_of(torch.uint8, shape).to(dev), tiles_of(torch.uint8, shape).flip(0).contiguous().to(dev)
    first, second = rows_t(row_sets(shape, size)[0], dev), rows_t(row_sets(shape, size)[1], dev)
    first_g, second_g = grids_t(grids_of(size, cell), dev), grids_t(grids_of(size, cell), dev).flip(0).contiguous() * 0.5
    aug = ElasticAugment(cell=cell, normalize_to_0_1=False, size=size)
    mask_of = lambda t: (t[:, 0] > 128).to(torch.uint8)  # noqa: E731
    call = (lambda t, g, r, m: aug(t, g, r, mask=m)) if with_mask else (lambda t, g, r, m: (aug(t, g, r), None))
    want_first, want_second = call(first_x, first_g, first, mask_of(first_x)), call(second_x, second_g, second, mask_of(second_x))
    assert not torch.equal(want_first[0], want_second[0])
    x, grids, buf, m = first_x.clone(), first_g.clone(), first.clone(), mask_of(first_x)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        call(x, grids, buf, m)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call(x, grids, buf, m)
        types, roots, edges = graph_nodes(dev)
    # kernel nodes only (hipGraphNodeTypeKernel = 0): ONE for the tiles, two with a mask, in a single branch; no memset node (2), no copy (1)
    assert types == ([0, 0] if with_mask else [0]), types
    assert roots == 1 and edges == (1 if with_mask else 0)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], want_first[0]) and (not with_mask or torch.equal(out[1], want_first[1]))
    buf.copy_(second)
    grids.copy_(second_g)
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
    grids = torch.ones((3, 2, *elastic_grid_shape((33, 31), 16)), dtype=torch.float32, device=dev)
    code, stream, bad = _native.DTYPE_CODES[torch.uint8], _native.stream_ptr(dev), _native.SX_ERR_BAD_ARG
    p = lambda t: t.data_ptr()      # noqa: E731

    def warp(images=p(x), to=p(out), dtype=code, n=3, h=33, w=31, oh=33, ow=31, r=p(rows), n_rows=3, g=p(grids), n_grids=3, cell=16, interpolation=BILINEAR, border=MIRROR, fill=0.0, flags=0):
        return lib.sx_elastic_warp(images, to, dtype, n, h, w, oh, ow, r, n_rows, g, n_grids, cell, interpolation, border, fill, flags, stream)

    def warp_mask(m=p(mask), to=p(mask_out), n=3, h=33, w=31, oh=33, ow=31, r=p(rows), n_rows=3, g=p(grids), n_grids=3, cell=16, border=CONSTANT, fill=0):
        return lib.sx_elastic_warp_mask(m, to, n, h, w, oh, ow, r, n_rows, g, n_grids, cell, border, fill, stream)

    for kwargs, word in (({"images": None}, "null"), ({"to": None}, "null"), ({"r": None}, "null"), ({"g": None}, "grids pointer is null"), ({"h": -33}, "positive"), ({"n": -3}, "positive"),
                         ({"oh": 0}, "positive"), ({"ow": -1}, "positive"), ({"n_rows": 2}, "n_rows"), ({"n_grids": 2}, "n_grids"), ({"cell": 3}, "cell"), ({"cell": 4097}, "cell"),
                         ({"interpolation": 2}, "interpolation"), ({"border": 2}, "border"), ({"fill": NAN}, "fill"), ({"fill": INF}, "fill"), ({"flags": 1 << 20}, "flags"),
                         ({"flags": OUT_FLAG[torch.bfloat16] | OUT_FLAG[torch.float16]}, "one of the two")):
        assert warp(**kwargs) == bad and word in _native.last_error(lib), kwargs
    assert warp(dtype=17) == _native.SX_ERR_DTYPE
    for kwargs, word in (({"m": None}, "null"), ({"to": None}, "null"), ({"r": None}, "null"), ({"g": None}, "null"), ({"w": 0}, "positive"), ({"oh": -2}, "positive"), ({"n_rows": 2}, "n_rows"),
                         ({"n_grids": 0}, "n_grids"), ({"cell": 0}, "cell"), ({"border": -1}, "border"), ({"fill": 256}, "0..255"), ({"fill": -1}, "0..255")):
        assert warp_mask(**kwargs) == bad and word in _native.last_error(lib), kwargs
    torch.cuda.synchronize(dev)
    assert bool((out == 7).all()) and bool((mask_out == 7).all())
