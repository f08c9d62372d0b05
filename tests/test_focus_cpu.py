"""Focus measurement without a GPU: the numpy restatement the GPU tests compare with is pinned to scipy's Laplacian and Sobel filters
(mode="mirror") and to the grey rule on every level; FocusStatistics' arithmetic (pool, total, the variance against exact rationals, sharp)
on hand-made integers; every refusal with its full text, in Python and at the C ABI; and "it matters": a 3 x 3 box blur cuts the
Laplacian variance of real tissue to less than a third."""
from __future__ import annotations

import ctypes
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import FocusStatistics, _native, cells_mask, focus_mask, focus_statistics, grey_map
from tests import _focus_numpy as fn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_grey_map": 8, "sx_focus_statistics": 11, "sx_focus_statistics_masked": 12, "sx_cells_mask": 10}
NAMES = ("FocusDetection", "FocusStatistics", "cells_mask", "focus_mask", "focus_statistics", "grey_map")
FAKE, FAKE2, FAKE3 = 1 << 40, 1 << 41, 3 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
BAD_SIDES = (1, 4, 7, 9, 12, 24, 48, 65, 96, 100, 130, -8, -64)
SIDES_TEXT = "block sides must each be 8, 16, 32, 64 or a multiple of 64, got (%d, %d)"


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.require_diag().sx_version() == 1
    for name in NAMES:
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.focus, name)
    assert fn.BLOCK == (64, 64) and "constexpr int kFocusRows = 64;" in (ROOT / "stainx_amd" / "csrc" / "focus.hpp").read_text()


# ------------------------------------------------------------------ the restatement IS scipy's
def grey_cases():
    rng = np.random.default_rng(11)
    yield "real", fn.grey_map(fn.real_crop())
    for shape in fn.SMALL_SHAPES + ((2, 9, 13),):
        yield shape, rng.integers(0, 256, shape, dtype=np.uint8)
    yield "main", fn.grey_map(fn.tiles_u8())


def test_numpy_stencils_are_scipy_mirror():
    import scipy.ndimage as ndi      # (a plain import: without scipy this test FAILS -- it is the one independent check of the restatement the GPU tests compare with)

    for what, grey in grey_cases():
        lap, ten = fn.stencils(grey)
        assert lap.dtype == np.int64 and ten.dtype == np.int64
        for i, tile in enumerate(grey.astype(np.int64)):      # (a tile at a time: tiles never see each other)
            assert np.array_equal(lap[i], ndi.laplace(tile, mode="mirror")), (what, i)
            gx, gy = ndi.sobel(tile, axis=1, mode="mirror"), ndi.sobel(tile, axis=0, mode="mirror")
            assert np.array_equal(ten[i], gx * gx + gy * gy), (what, i)
        assert np.abs(lap).max() <= fn.MAX_L and ten.max() <= fn.MAX_T
    # the extremes are reached: a checkerboard of 0 and 255 has |L| = 1020 everywhere; a step edge has |G| = 1020
    yy, xx = np.meshgrid(np.arange(6), np.arange(7), indexing="ij")
    lap, ten = fn.stencils(np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)[None])
    assert np.abs(lap).min() == fn.MAX_L and ten.max() == 0
    lap, ten = fn.stencils(np.where(xx < 3, 0, 255).astype(np.uint8)[None])
    assert ten.max() == 1020 * 1020
    corner = np.zeros((1, 5, 5), dtype=np.uint8)
    corner[0, 3:, 3:] = 255
    assert fn.stencils(corner)[1].max() <= fn.MAX_T
    # a length-1 axis maps to 0: the tile's own value on every side
    assert np.array_equal(fn.stencils(np.array([[[9]]], dtype=np.uint8))[0], [[[0]]])
    row = np.array([[[1, 5, 2, 200, 0, 7, 9]]], dtype=np.uint8)
    assert np.array_equal(fn.stencils(row)[0][0, 0], [2 * 5 - 2 * 1, 1 + 2 - 10, 5 + 200 - 4, 2 + 0 - 400, 200 + 7, 0 + 9 - 14, 2 * 7 - 18])


def test_grey_rule_on_every_level_and_at_the_rounding_boundaries():
    ladder = np.arange(256, dtype=np.int64)
    zero = np.zeros(256, dtype=np.int64)
    for channel, weight in enumerate((4899, 9617, 1868)):
        levels = [zero, zero, zero]
        levels[channel] = ladder
        got = fn.grey_of_levels(*levels)
        assert got.tolist() == [int(Fraction(weight * v, 16384) + Fraction(1, 2)) for v in range(256)], channel      # rounded half up, exactly
    assert fn.grey_of_levels(ladder, ladder, ladder).tolist() == list(range(256))      # the weights sum to 16384: grey stays grey
    assert 4899 + 9617 + 1868 == 16384
    # around a rounding boundary: 9617 g + 8192 crosses a multiple of 16384 between g = 22 (13.41 -> 13) and g = 23 (14.0004 -> 14)
    g = np.array([22, 23], dtype=np.int64)
    assert fn.grey_of_levels(np.zeros(2, dtype=np.int64), g, np.zeros(2, dtype=np.int64)).tolist() == [13, 14]
    # exact halves do not occur with one channel, but do with mixtures: 4899 r + 9617 g + 1868 b = 16384 k + 8192 rounds UP
    found = [(r, gg, b) for r in range(0, 256, 5) for gg in range(0, 256, 3) for b in range(256) if (4899 * r + 9617 * gg + 1868 * b) % 16384 == 8192][:3]
    for r, gg, b in found:
        total = 4899 * r + 9617 * gg + 1868 * b
        assert int(fn.grey_of_levels(np.array(r), np.array(gg), np.array(b))) == total // 16384 + 1
    # the map: uint8 as it is, floats by their levels, NaN pixels 0, both layouts
    u8 = np.stack([ladder, ladder[::-1], (ladder * 7) % 256]).astype(np.uint8)[None, :, None, :]      # (1, 3, 1, 256)
    want = fn.grey_of_levels(u8[0, 0], u8[0, 1], u8[0, 2]).astype(np.uint8)[None]
    assert np.array_equal(fn.grey_map(u8), want)
    assert np.array_equal(fn.grey_map((u8 / 255.0).astype(np.float32)), want) and np.array_equal(fn.grey_map(u8 / 255.0), want)
    assert np.array_equal(fn.grey_map(np.moveaxis(u8, 1, -1), channel_axis=-1), want)
    floats = (u8 / 255.0).astype(np.float32)
    floats[0, 1, 0, 5] = np.nan
    got = fn.grey_map(floats)
    assert got[0, 0, 5] == 0 and np.array_equal(np.delete(got, 5, axis=2), np.delete(want, 5, axis=2))


def test_statistics_cells_add_up_and_masks_select():
    grey = fn.grey_map(fn.tiles_u8())
    whole = fn.statistics_of_grey(grey)
    lap, ten = fn.stencils(grey)
    assert whole.shape == (4, 3, 1, 1) and whole[0].reshape(-1).tolist() == [150 * 203] * 3
    assert np.array_equal(whole[1].reshape(-1), lap.sum(axis=(1, 2))) and np.array_equal(whole[2].reshape(-1), (lap * lap).sum(axis=(1, 2))) and np.array_equal(whole[3].reshape(-1), ten.sum(axis=(1, 2)))
    assert whole[2, 1, 0, 0] == 0 and whole[3, 1, 0, 0] == 0      # the constant tile
    assert whole[2, 2, 0, 0] == 150 * 203 * 1020 * 1020 and whole[3, 2, 0, 0] == 0      # the checkerboard: |L| = 1020 at every pixel, no gradient
    for block in fn.BLOCKS[1:]:
        grid = fn.statistics_of_grey(grey, block)
        assert grid.shape == (4, 3, -(-150 // block[0]), -(-203 // block[1]))
        assert np.array_equal(grid.sum(axis=(2, 3), keepdims=True), whole), block
    assert np.array_equal(fn.statistics_of_grey(grey, pooled=True), whole.sum(axis=1, keepdims=True))
    mask = fn.tiles_mask()
    masked = fn.statistics_of_grey(grey, (16, 32), mask)
    assert np.array_equal(masked[0].sum(axis=(1, 2)), (mask != 0).sum(axis=(1, 2)))
    assert np.array_equal(masked[1, 0, 2, 3], lap[0, 32:48, 96:128][mask[0, 32:48, 96:128] != 0].sum())      # neighbours are read whatever the mask says
    assert np.array_equal(fn.statistics_of_grey(grey, (8, 8), fn.tiles_mask(kind="ones")), fn.statistics_of_grey(grey, (8, 8)))
    assert not fn.statistics_of_grey(grey, (8, 8), fn.tiles_mask(kind="zeros")).any()
    cells = np.arange(3 * 3 * 4).reshape(3, 3, 4) % 3
    big = fn.cells_mask(cells, 150, 203, (64, 64))
    assert big.shape == (3, 150, 203) and big[0, 63, 64] == (cells[0, 0, 1] != 0) and big[2, 149, 202] == (cells[2, 2, 3] != 0)
    assert np.array_equal(fn.cells_mask(cells, 150, 203, (64, 64), mask), big & (mask != 0))


# ------------------------------------------------------------------ FocusStatistics on hand-made integers
def stats_of(pixels, sums, squares, gradients) -> FocusStatistics:
    return FocusStatistics(*(torch.tensor(v, dtype=torch.int64).reshape(1, 1, -1) for v in (pixels, sums, squares, gradients)))


def test_pool_and_total_add_integers_exactly():
    big = 1 << 61
    a = stats_of([5, 0, big], [-7, 0, -big], [49, 0, big], [3, 0, 1])
    b = stats_of([1, 0, big], [7, 0, big - 1], [1, 0, big], [1, 0, big])
    pooled = FocusStatistics.pool(a, b)
    assert pooled.pixels.tolist() == [[[6, 0, 2 * big]]] and pooled.sums.tolist() == [[[0, 0, -1]]]
    assert pooled.squares.tolist() == [[[50, 0, 2 * big]]] and pooled.gradients.tolist() == [[[4, 0, big + 1]]]
    assert all(t.dtype == torch.int64 and t.shape == (1, 1, 3) for t in pooled)
    assert all(torch.equal(x, y) for x, y in zip(FocusStatistics.pool(a), a))
    total = a.total()
    assert all(t.shape == (1, 1, 1) for t in total) and total.pixels.item() == 5 + big and total.sums.item() == -7 - big
    grid = FocusStatistics(*(torch.arange(24, dtype=torch.int64).reshape(2, 3, 4) * (k + 1) for k in range(4)))
    assert grid.total().pixels.reshape(-1).tolist() == [66, 210] and grid.total().gradients.reshape(-1).tolist() == [264, 840]
    with pytest.raises(ValueError, match=r"^pool needs at least one FocusStatistics$"):
        FocusStatistics.pool()
    with pytest.raises(ValueError, match=r"^pool takes statistics of equal shapes, got \(1, 1, 3\) and \(2, 3, 4\)$"):
        FocusStatistics.pool(a, grid)
    with pytest.raises(ValueError, match=r"^pool takes FocusStatistics, got tuple$"):
        FocusStatistics.pool(a, (1, 2, 3, 4))


def test_variance_is_within_1e_9_of_the_exact_rational():
    # (pixels, sum L, sum L^2): small cells, an empty one, a constant one, and slides' worth of pixels -- pixels * squares far beyond int64
    cases = [(1, 5, 25), (2, 0, 2 * 1020 * 1020), (3, -7, 49), (4096, 1234, 4096 * 777 + 5), (0, 0, 0), (150 * 203, 0, 150 * 203 * 1020 * 1020),
             (1 << 40, 3 * (1 << 40) + 12345, 300_000 * (1 << 40) + 987), (1 << 42, -(1 << 43) - 99, 1_040_400 * (1 << 41)), ((1 << 40) + 1, -17, 1234 * (1 << 40) + 77)]
    assert max(p * q for p, _, q in cases) > (1 << 63) * (1 << 20)
    stats = stats_of([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[2] * 2 for c in cases])
    var, ten = stats.laplacian_variance(), stats.tenengrad()
    assert var.dtype == torch.float64 and var.shape == (1, 1, len(cases)) and ten.dtype == torch.float64
    for i, (pixels, sums, squares) in enumerate(cases):
        exact = fn.variance_exact(pixels, sums, squares)
        if exact is None:
            assert torch.isnan(var[0, 0, i]) and torch.isnan(ten[0, 0, i])
            continue
        assert exact >= 0
        assert abs(Fraction(var[0, 0, i].item()) - exact) <= Fraction(1, 10 ** 9), (i, var[0, 0, i].item(), float(exact))
        assert abs(Fraction(ten[0, 0, i].item()) - Fraction(2 * squares, pixels)) <= Fraction(1, 10 ** 9), i


def test_sharp_thresholds_pixels_and_variance_and_nan_is_false():
    #           empty   one pixel   var 100 on 8 px      var 99.99..    var 100 on 7 px
    stats = stats_of([0, 1, 8, 8, 7], [0, 3, 0, 0, 0], [0, 9, 800, 799, 700], [0, 0, 0, 0, 0])
    assert stats.laplacian_variance()[0, 0, 1:].tolist() == [0.0, 100.0, 99.875, 100.0]
    cells = stats.sharp(100.0)
    assert cells.dtype == torch.uint8 and cells.shape == (1, 1, 5) and cells.reshape(-1).tolist() == [0, 0, 1, 0, 1]
    assert stats.sharp(100, min_pixels=8).reshape(-1).tolist() == [0, 0, 1, 0, 0]
    assert stats.sharp(0.0).reshape(-1).tolist() == [0, 1, 1, 1, 1]                  # NaN >= 0 is false: the empty cell stays 0
    assert stats.sharp(-1.0, min_pixels=0).reshape(-1).tolist() == [0, 1, 1, 1, 1]   # ... even when no pixel is asked for
    assert stats.sharp(float("inf")).reshape(-1).tolist() == [0] * 5
    for bad in (None, "100", True, float("nan"), [1.0]):
        with pytest.raises(ValueError, match=r"^min_variance must be a number, got "):
            stats.sharp(bad)
    for bad in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match=r"^min_pixels must be a non-negative integer, got "):
            stats.sharp(1.0, min_pixels=bad)


# ------------------------------------------------------------------ refusals, with their full texts
def test_python_refusals_before_gpu_work():
    images = torch.zeros(2, 3, 8, 8)
    block_text = r"^block must be None or \(bh, bw\) with each side one of 8, 16, 32, 64 or a multiple of 64, got %s$"
    for bad in ((8,), (8, 8, 8), 8, "8x8", (8.0, 8), (True, 8), (0, 0), (64, 0)) + tuple((s, 64) for s in BAD_SIDES) + tuple((8, s) for s in BAD_SIDES):
        with pytest.raises(ValueError, match=block_text % re.escape(repr(bad))):
            focus_statistics(images, block=bad)
        with pytest.raises(ValueError, match=r"^block must be \(bh, bw\) with each side one of 8, 16, 32, 64 or a multiple of 64, got " + re.escape(repr(bad)) + "$"):
            focus_mask(images, 10.0, block=bad)
        with pytest.raises(ValueError, match=r"^block must be \(bh, bw\) with each side one of 8, 16, 32, 64 or a multiple of 64, got " + re.escape(repr(bad)) + "$"):
            cells_mask(torch.zeros(2, 1, 1, dtype=torch.uint8), 8, 8, bad)
    with pytest.raises(ValueError, match=r"^block must be \(bh, bw\) with each side one of 8, 16, 32, 64 or a multiple of 64, got None$"):
        focus_mask(images, 10.0, block=None)
    for good in ((8, 8), (16, 64), (64, 128), (640, 32), [8, 16]):
        assert stainx_amd.focus.check_block(good) == tuple(good)
    with pytest.raises(ValueError, match=r"^pooled=True pools whole tiles: it goes with block=None, got block=\(64, 64\)$"):
        focus_statistics(images, block=(64, 64), pooled=True)
    for call, name in ((grey_map, "grey_map"), (focus_statistics, "focus_statistics"), (lambda x, **k: focus_mask(x, 10.0, **k), "focus_mask")):
        for value in (torch.zeros(3, 8, 8), np.zeros((2, 3, 8, 8))):
            with pytest.raises(ValueError, match=f"^{name} expects a 4-D image tensor, got "):
                call(value)
        with pytest.raises(ValueError, match=f"^{name} expects 3 channels on axis 1, got shape " + re.escape("(2, 4, 8, 8)") + "$"):
            call(torch.zeros(2, 4, 8, 8))
        with pytest.raises(ValueError, match=f"^{name} expects 3 channels on axis -1, got shape " + re.escape("(2, 3, 8, 8)") + "$"):
            call(images, channel_axis=-1)
        with pytest.raises(ValueError, match=r"^Unsupported channel_axis=2$"):
            call(images, channel_axis=2)
    # masks: the texts every masked call has
    with pytest.raises(ValueError, match=r"^mask must be None or one of \['luminosity'\], got 'otsu'$"):
        focus_statistics(images, mask="otsu")
    with pytest.raises(ValueError, match=r"^mask must be None, 'luminosity' or a uint8 / bool tensor, got ndarray$"):
        focus_statistics(images, mask=np.ones((2, 8, 8), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"^an explicit mask goes with images on the GPU, got images on cpu$"):
        focus_statistics(images, mask=torch.ones(2, 8, 8, dtype=torch.uint8))
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"^luminosity_threshold must lie in \(0, 1\), got "):
            focus_statistics(images, mask="luminosity", luminosity_threshold=bad)
    with pytest.raises(ValueError, match=r"^luminosity_threshold must be a number in \(0, 1\), got None$"):
        focus_mask(images, 10.0, luminosity_threshold=None)
    for bad in (None, "10", float("nan"), True):
        with pytest.raises(ValueError, match=r"^min_variance must be a number, got "):
            focus_mask(images, bad)
    for bad in (-1, 2.5, "4", True):
        with pytest.raises(ValueError, match=r"^min_pixels must be a non-negative integer, got "):
            focus_mask(images, 10.0, min_pixels=bad)
    # cells_mask
    cells = torch.zeros(2, 3, 4, dtype=torch.uint8)
    for h, w, name in ((0, 203, "height"), (150, -1, "width"), (150.0, 203, "height"), (150, True, "width")):
        with pytest.raises(ValueError, match=f"^{name} must be a positive integer, got "):
            cells_mask(cells, h, w, (64, 64))
    for bad in (torch.zeros(2, 3, 4), torch.zeros(3, 4, dtype=torch.uint8), np.zeros((2, 3, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r"^cells must be a uint8 / bool tensor \(N, gh, gw\), got "):
            cells_mask(bad, 150, 203, (64, 64))
    with pytest.raises(ValueError, match=r"^cells must be \(N, gh, gw\) with \(gh, gw\) = \(5, 4\) for 150 x 203 pixels in 32 x 64 cells, got \(2, 3, 4\)$"):
        cells_mask(cells, 150, 203, (32, 64))
    with pytest.raises(ValueError, match=r"^cells device must be a GPU, got cpu$"):
        cells_mask(cells, 150, 203, (64, 64))


def test_c_abi_refusals_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        def gmap(images=FAKE, dtype=u8, n=4, h=64, w=64, last=0, out=FAKE2):
            return lib.sx_grey_map(images, dtype, n, h, w, last, out, None)

        def stat(images=FAKE, dtype=u8, n=4, h=64, w=64, last=0, bh=0, bw=0, pooled=0, out=FAKE2):
            return lib.sx_focus_statistics(images, dtype, n, h, w, last, bh, bw, pooled, out, None)

        def mstat(images=FAKE, dtype=u8, n=4, h=64, w=64, last=0, bh=0, bw=0, pooled=0, mask=FAKE3, out=FAKE2):
            return lib.sx_focus_statistics_masked(images, dtype, n, h, w, last, bh, bw, pooled, mask, out, None)

        def cmask(cells=FAKE, n=4, h=64, w=64, bh=64, bw=64, mask=None, out=FAKE2, counts=FAKE3):
            return lib.sx_cells_mask(cells, n, h, w, bh, bw, mask, out, counts, None)

        def said():
            return _native.last_error(lib)

        assert gmap(images=None) == BAD and said() == "images pointer is null"
        assert gmap(out=None) == BAD and said() == "levels_out pointer is null"
        for kwargs in ({"n": 0}, {"n": -2}, {"h": -1}, {"w": 0}):
            assert gmap(**kwargs) == BAD and said() == "images must have positive sizes", kwargs
        assert gmap(n=1 << 40) == BAD and said() == f"too many tiles for one call: {1 << 40}"
        assert gmap(dtype=17) == DTYPE and said() == "unsupported dtype code 17"
        for call in (stat, mstat):
            assert call(images=None) == BAD and said() == "images pointer is null"
            assert call(out=None) == BAD and said() == "statistics_out pointer is null"
            for kwargs in ({"n": 0}, {"n": -2}, {"h": -1}, {"w": 0}):
                assert call(**kwargs) == BAD and said() == "images must have positive sizes", kwargs
            for side in BAD_SIDES + (0,):      # (one side 0 is no whole tile)
                assert call(bh=side, bw=64) == BAD and said() == SIDES_TEXT % (side, 64), side
                assert call(bh=8, bw=side) == BAD and said() == SIDES_TEXT % (8, side), side
            assert call(bh=64, bw=64, pooled=1) == BAD and said() == "pooled statistics take the whole tile as the cell (block 0 x 0), got (64, 64)"
            assert call(n=1 << 40, h=1 << 20, w=1 << 20) == BAD and said() == "images too large for one call"
            assert call(dtype=17) == DTYPE and said() == "unsupported dtype code 17"
            assert call(dtype=-1, bh=128, bw=64) == DTYPE
        assert mstat(mask=None) == BAD and said() == "mask pointer is null (the masked calls take explicit masks: one byte per pixel, (N, H, W))"
        assert cmask(cells=None) == BAD and said() == "cells pointer is null"
        assert cmask(out=None, counts=None) == BAD and said() == "mask_out and tile_counts_out are both null"
        for kwargs in ({"n": 0}, {"n": -2}, {"h": -1}, {"w": 0}):
            assert cmask(**kwargs) == BAD and said() == "masks must have positive sizes", kwargs
        assert cmask(n=1 << 40) == BAD and said() == f"too many tiles for one call: {1 << 40}"
        for side in BAD_SIDES + (0,):
            assert cmask(bh=side) == BAD and said() == SIDES_TEXT % (side, 64), side
            assert cmask(bw=side) == BAD and said() == SIDES_TEXT % (64, side), side


# ------------------------------------------------------------------ it matters
def test_a_box_blur_cuts_the_variance_of_real_tissue_to_less_than_a_third():
    sharp = fn.real_crop()      # (3, 3, 150, 203): the crop tests/_saturation_numpy.real_saturation uses
    blurred = fn.box_blur(sharp, 3)
    a, b = fn.statistics(sharp), fn.statistics(blurred)
    for index in np.ndindex(a.shape[1:]):
        var_sharp = fn.variance_exact(*(int(a[k][index]) for k in range(3)))
        var_blurred = fn.variance_exact(*(int(b[k][index]) for k in range(3)))
        print(f"tile {index[0]}: Laplacian variance {float(var_sharp):.1f} sharp, {float(var_blurred):.1f} blurred ({float(var_sharp / var_blurred):.2f}x)")
        assert var_blurred * 3 < var_sharp, (index, float(var_sharp), float(var_blurred))
        assert Fraction(int(b[3][index]), int(b[0][index])) < Fraction(int(a[3][index]), int(a[0][index])), index      # the Tenengrad falls too
