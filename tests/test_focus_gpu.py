"""Focus measurement on the GPU, every result an integer and every check exact (torch.equal with the numpy restatements of
tests/_focus_numpy.py, which the CPU tests pin to scipy): the grey map over element types and layouts; the statistics on shapes with axes of
length 1 and 2, on a shape of two full 64 x 64 blocks and a ragged remainder both ways, and on exactly one and two blocks (the 4-wide
loads); every kind of cell, adding up exactly; masks; workspace etiquette; a captured focus_mask that reads the images at replay;
cells_mask; focus_mask against its own steps; and the refusals of the C ABI, which leave the output untouched."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import FocusDetection, FocusStatistics, Macenko, _native, cells_mask, focus_mask, focus_statistics, grey_map, level_histogram, median_filter, synth, tissue_mask
from tests import _focus_numpy as fn
from tests import _saturation_numpy as sn
from tests.conftest import TORCH_DTYPES
from tests.test_tissue_mask_gpu import unaligned_copy

pytestmark = pytest.mark.gpu

LAYOUTS = ("nchw", "nhwc", "unaligned")
DTYPE_NAMES = ["u8", "f16", "bf16", "f32", "f64"]
POISON = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def in_layout(x: torch.Tensor, layout: str) -> tuple[torch.Tensor, int]:
    if layout == "nhwc":
        return x.permute(0, 2, 3, 1).contiguous(), -1
    return (unaligned_copy(x) if layout == "unaligned" else x), 1


def words(stats: FocusStatistics) -> torch.Tensor:
    assert isinstance(stats, FocusStatistics)
    for t in stats:
        assert t.dtype == torch.int64 and t.shape == stats.pixels.shape and t.device.type == "cuda"
    return torch.stack(list(stats)).cpu()


def on(dev, array: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(array)).to(dev)      # (a copy: the shared inputs are read-only)


# ------------------------------------------------------------------ 1. the grey map
def assert_grey(x_cpu: torch.Tensor, dev, what) -> None:
    want = torch.from_numpy(fn.grey_map(fn.as_numpy(x_cpu)))
    for layout in LAYOUTS:
        x, axis = in_layout(x_cpu.to(dev), layout)
        got = grey_map(x, channel_axis=axis)
        assert got.dtype == torch.uint8 and got.shape == want.shape and got.device == x.device, (what, layout)
        assert torch.equal(got.cpu(), want), (what, layout)


@pytest.mark.parametrize("name", DTYPE_NAMES)
def test_grey_map_dtypes_layouts_shapes(dev, name):
    dt = TORCH_DTYPES[name]
    for kind in ("he", "noise"):
        for index in range(len(sn.MAP_SHAPES)):      # (3, 30, 30): packs of four; (2, 33, 47) and (1, 5, 4): single elements
            assert_grey(synth.as_dtype(sn.map_tiles_u8(kind, index), dt), dev, (kind, index, name))
    assert_grey(synth.as_dtype(sn.ladder_u8(), dt), dev, ("ladder", name))
    if name != "u8":
        x = sn.special_floats(dt)
        assert_grey(x, dev, ("special", name))
        got = grey_map(x.to(dev))[0].cpu()
        assert got[0, 0].item() == 0 and got[0, 5].item() == 0      # a NaN in one channel, or in all: Y = 0
        assert got[0, 1].item() == (4899 * 255 + 1868 * 128 + 8192) >> 14      # (inf, 0, 0.5): inf clamps to 255
    empty = grey_map(torch.empty((0, 3, 5, 7), dtype=dt, device=dev))
    assert empty.shape == (0, 5, 7) and empty.dtype == torch.uint8


def test_grey_map_feeds_the_level_functions(dev):
    x = on(dev, fn.tiles_u8())
    levels = grey_map(x)
    want = fn.grey_map(fn.tiles_u8())
    assert torch.equal(level_histogram(levels).counts.cpu(), torch.from_numpy(sn.histogram(want)))
    assert torch.equal(median_filter(levels, 3).cpu(), torch.from_numpy(sn.median(want, 3)))


# ------------------------------------------------------------------ 2. the statistics
@pytest.mark.parametrize("shape", fn.SMALL_SHAPES, ids=str)
def test_statistics_small_shapes(dev, shape):
    tiles = fn.tiles_u8(shape)
    for layout in LAYOUTS:
        x, axis = in_layout(on(dev, tiles), layout)
        assert torch.equal(words(focus_statistics(x, channel_axis=axis)), fn.as_torch(fn.want(shape))), layout
        assert torch.equal(words(focus_statistics(x, channel_axis=axis, block=(8, 8))), fn.as_torch(fn.want(shape, (8, 8)))), layout
        assert torch.equal(words(focus_statistics(x, channel_axis=axis, pooled=True)), fn.as_torch(fn.want(shape, None, None, True))), layout
    mask = (np.arange(int(np.prod(shape))).reshape(shape) % 3 != 1).astype(np.uint8)
    assert torch.equal(words(focus_statistics(on(dev, tiles), mask=on(dev, mask))), fn.as_torch(fn.statistics(tiles, None, mask)))


def test_statistics_main_shape_every_layout(dev):
    n, h, w = fn.MAIN_SHAPE
    assert h > 2 * fn.BLOCK[0] and h % fn.BLOCK[0] and w > 2 * fn.BLOCK[1] and w % fn.BLOCK[1] and w % 4      # halos across workgroups, ragged edges, single elements
    tiles = fn.tiles_u8()
    want = fn.as_torch(fn.want())
    assert want[2, 1, 0, 0] == 0 and want[2, 2, 0, 0] == h * w * fn.MAX_L ** 2      # the constant tile and the checkerboard: the extreme L at every pixel
    for layout in LAYOUTS:
        x, axis = in_layout(on(dev, tiles), layout)
        assert torch.equal(words(focus_statistics(x, channel_axis=axis)), want), layout
    # tiles never see each other: a tile measured alone has the integers it has in the batch
    for i in range(n):
        assert torch.equal(words(focus_statistics(on(dev, tiles[i:i + 1]))), want[:, i:i + 1]), i
    # the extreme T: a step edge in every channel
    yy, xx = np.meshgrid(np.arange(70), np.arange(130), indexing="ij")
    step = np.broadcast_to(np.where((xx // 3 + yy // 5) % 2 == 0, 0, 255).astype(np.uint8), (2, 3, 70, 130))
    got = words(focus_statistics(on(dev, step), block=(8, 8)))
    assert torch.equal(got, fn.as_torch(fn.statistics(step, (8, 8)))) and fn.stencils(fn.grey_map(step))[1].max() >= fn.MAX_L ** 2
    empty = focus_statistics(torch.empty((0, 3, 5, 7), dtype=torch.uint8, device=dev), block=(8, 8))
    assert empty.pixels.shape == (0, 1, 1)


@pytest.mark.parametrize("shape", fn.ALIGNED_SHAPES, ids=str)
def test_statistics_whole_blocks_take_the_wide_loads(dev, shape):
    assert shape[1] % fn.BLOCK[0] == 0 and shape[2] % fn.BLOCK[1] == 0
    tiles = fn.tiles_u8(shape)
    x = on(dev, tiles)
    assert x.data_ptr() % 16 == 0
    for block in (None, (8, 8), (16, 32), (64, 64), (128, 64), (64, 192)):
        want = fn.as_torch(fn.want(shape, block))
        assert torch.equal(words(focus_statistics(x, block=block)), want), block
        assert torch.equal(words(focus_statistics(unaligned_copy(x), block=block)), want), block                                   # single elements: the same integers
        assert torch.equal(words(focus_statistics(x.permute(0, 2, 3, 1).contiguous(), block=block, channel_axis=-1)), want), block
    # a width that is a multiple of 4 and no multiple of the block: packs up to the tile's edge, the reflected column behind it
    for width in (60, 68, 124):
        part = np.ascontiguousarray(fn.tiles_u8((2, 64, 128))[:, :, :37, :width])
        assert torch.equal(words(focus_statistics(on(dev, part), block=(8, 16))), fn.as_torch(fn.statistics(part, (8, 16)))), width


@pytest.mark.parametrize("block", fn.BLOCKS, ids=str)
def test_cells_add_up_exactly(dev, block):
    x = on(dev, fn.tiles_u8())
    stats = focus_statistics(x, block=block)
    n, h, w = fn.MAIN_SHAPE
    assert stats.pixels.shape == ((n, 1, 1) if block is None else (n, -(-h // block[0]), -(-w // block[1])))
    assert torch.equal(words(stats), fn.as_torch(fn.want(fn.MAIN_SHAPE, block)))
    whole = focus_statistics(x)
    assert torch.equal(words(stats.total()), words(whole))                                       # the grid cells add up to the block=None row
    pooled = focus_statistics(x, pooled=True)
    assert pooled.pixels.shape == (1, 1, 1)
    assert torch.equal(words(pooled), words(whole).sum(dim=1, keepdim=True))                     # the block=None rows add up to the pooled row
    assert torch.equal(words(pooled), fn.as_torch(fn.want(fn.MAIN_SHAPE, None, None, True)))
    assert torch.equal(words(FocusStatistics.pool(*(focus_statistics(x[i:i + 1], pooled=True) for i in range(n)))), words(pooled))


# ------------------------------------------------------------------ 3. masks
@pytest.mark.parametrize("block", [None, (8, 8), (64, 64), (128, 64)], ids=str)
def test_masks(dev, block):
    tiles = fn.tiles_u8()
    x = on(dev, tiles)
    mask = on(dev, fn.tiles_mask())
    want = fn.as_torch(fn.want(fn.MAIN_SHAPE, block, "random"))
    assert torch.equal(words(focus_statistics(x, block=block, mask=mask)), want)
    assert torch.equal(words(focus_statistics(x, block=block, mask=mask != 0)), want)             # bool: the same bytes
    assert torch.equal(words(focus_statistics(x, block=block, mask=mask[:, None])), want)         # (N, 1, H, W)
    shifted = unaligned_copy(mask)                                                                # a mask offset by one byte
    assert shifted.data_ptr() % 4 != 0
    assert torch.equal(words(focus_statistics(x, block=block, mask=shifted)), want)
    assert torch.equal(words(focus_statistics(x.permute(0, 2, 3, 1).contiguous(), block=block, mask=mask, channel_axis=-1)), want)
    plain = words(focus_statistics(x, block=block))
    assert torch.equal(words(focus_statistics(x, block=block, mask=torch.ones_like(mask))), plain)    # all ones: no mask, bit for bit
    none = focus_statistics(x, block=block, mask=torch.zeros_like(mask))
    assert not words(none).any() and torch.isnan(none.laplacian_variance()).all() and torch.isnan(none.tenengrad()).all()
    assert not none.sharp(0.0, min_pixels=0).any()
    if block is None:
        assert torch.equal(words(focus_statistics(x, mask=mask, pooled=True)), fn.as_torch(fn.want(fn.MAIN_SHAPE, None, "random", True)))


def test_masks_on_whole_blocks_take_the_wide_loads(dev):
    shape = fn.ALIGNED_SHAPES[1]
    x, mask = on(dev, fn.tiles_u8(shape)), on(dev, fn.tiles_mask(shape))
    assert mask.data_ptr() % 4 == 0 and shape[2] % 4 == 0
    for block in (None, (16, 32), (64, 64)):
        want = fn.as_torch(fn.want(shape, block, "random"))
        assert torch.equal(words(focus_statistics(x, block=block, mask=mask)), want), block
        assert torch.equal(words(focus_statistics(x, block=block, mask=unaligned_copy(mask))), want), block
        assert torch.equal(words(focus_statistics(unaligned_copy(x), block=block, mask=mask)), want), block


def test_luminosity_is_the_explicit_tissue_mask(dev):
    images = synth.background_stripes(synth.he_batch(3, 150, 203, seed0=11, scale_step=0.1))
    x = images.to(dev)
    for threshold in (0.8, 0.6):
        tissue, counts = tissue_mask(x, threshold)
        assert 0 < int(counts.sum()) < tissue.numel()
        for block in (None, (64, 64)):
            got = focus_statistics(x, block=block, mask="luminosity", luminosity_threshold=threshold)
            assert torch.equal(words(got), words(focus_statistics(x, block=block, mask=tissue))), (threshold, block)
            assert torch.equal(words(got), fn.as_torch(fn.statistics(images.numpy(), block, tissue.cpu().numpy()))), (threshold, block)
            assert torch.equal(got.total().pixels.reshape(-1), counts)
    nhwc = focus_statistics(x.permute(0, 2, 3, 1).contiguous(), mask="luminosity", channel_axis=-1)
    assert torch.equal(words(nhwc), words(focus_statistics(x, mask="luminosity")))


# ------------------------------------------------------------------ 4. element types
@pytest.mark.parametrize("name", DTYPE_NAMES)
def test_element_types_planar_and_nhwc(dev, name):
    dt = TORCH_DTYPES[name]
    u8 = torch.from_numpy(fn.tiles_u8().copy())
    x_cpu = synth.as_dtype(u8, dt)
    want_own = {block: fn.as_torch(fn.statistics(fn.as_numpy(x_cpu), block)) for block in (None, (16, 32))}      # the restatement on the stored elements
    for layout in LAYOUTS:
        x, axis = in_layout(x_cpu.to(dev), layout)
        for block, want in want_own.items():
            assert torch.equal(words(focus_statistics(x, block=block, channel_axis=axis)), want), (layout, block)
    wide = synth.as_dtype(torch.from_numpy(fn.tiles_u8(fn.ALIGNED_SHAPES[1]).copy()), dt)      # whole blocks: packs of four elements
    assert torch.equal(words(focus_statistics(wide.to(dev), block=(8, 8))), fn.as_torch(fn.statistics(fn.as_numpy(wide), (8, 8))))
    if name in ("f32", "f64"):      # a float tile equal to u8 / 255 has the uint8 tile's integers
        for unit in ((u8.to(torch.float32) / 255.0).to(dt), (u8.to(torch.float64) / 255.0).to(dt)):
            assert torch.equal(words(focus_statistics(unit.to(dev))), fn.as_torch(fn.want()))
    if name != "u8":
        special = sn.special_floats(dt)
        assert torch.equal(words(focus_statistics(special.to(dev))), fn.as_torch(fn.statistics(fn.as_numpy(special))))


# ------------------------------------------------------------------ 5. workspace etiquette
def raw_statistics(lib, x, block, pooled, out, mask=None, stream=None):
    n, _, h, w = x.shape
    bh, bw = block or (0, 0)
    stream = _native.stream_ptr(x.device) if stream is None else stream
    if mask is None:
        return lib.sx_focus_statistics(x.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, 0, bh, bw, int(pooled), out.data_ptr(), stream)
    return lib.sx_focus_statistics_masked(x.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, 0, bh, bw, int(pooled), mask.data_ptr(), out.data_ptr(), stream)


def test_poisoned_output_and_a_side_stream(dev):
    lib = _native.require()
    x, mask = on(dev, fn.tiles_u8()), on(dev, fn.tiles_mask())
    n, h, w = fn.MAIN_SHAPE
    for block in fn.BLOCKS:
        for pooled in ((False, True) if block is None else (False,)):
            for m, kind in ((None, None), (mask, "random")):
                want = fn.as_torch(fn.want(fn.MAIN_SHAPE, block, kind, pooled))
                out = torch.full((want.numel() + 2,), POISON, dtype=torch.int64, device=dev)      # a guard word on either side
                assert raw_statistics(lib, x, block, pooled, out[1:-1], m) == 0
                assert torch.equal(out[1:-1].cpu().view(want.shape), want), (block, pooled, kind)
                assert out[0].item() == POISON and out[-1].item() == POISON, (block, pooled, kind)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        first = focus_statistics(x, block=(64, 64), mask=mask)
        second = focus_statistics(x)
        det = focus_mask(x, 100.0, mask=mask)
    side.synchronize()
    assert torch.equal(words(first), fn.as_torch(fn.want(fn.MAIN_SHAPE, (64, 64), "random"))) and torch.equal(words(second), fn.as_torch(fn.want()))
    assert torch.equal(words(det.statistics), words(first))
    # twice into one buffer: the second call does not add to the first
    out = torch.full((4 * n,), POISON, dtype=torch.int64, device=dev)
    assert raw_statistics(lib, x, None, False, out) == 0 and raw_statistics(lib, x, None, False, out) == 0
    assert torch.equal(out.cpu().view(4, n, 1, 1), fn.as_torch(fn.want()))


# ------------------------------------------------------------------ 6. one captured graph
def test_captured_focus_mask_reads_the_images_at_replay(dev):
    a = synth.background_stripes(synth.he_batch(2, 150, 203, seed0=7, scale_step=0.1)).to(dev)
    b = on(dev, fn.tiles_u8()[:2])
    for block, mask in (((64, 64), "luminosity"), ((128, 64), None)):      # plain stores, and adds into cleared words: the clear must replay too
        cut = 50.0
        x = a.clone()
        focus_mask(x, cut, block=block, mask=mask)      # (warm-up: the library is loaded and every kernel has run once)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):      # a linear capture on one stream; a call that synchronised would fail it
            det = focus_mask(x, cut, block=block, mask=mask)
            whole = focus_statistics(x, pooled=True)
        for images in (b, a, b):      # (replayed more than once: words that were added into are cleared at every replay)
            x.copy_(images)
            graph.replay()
            torch.cuda.synchronize(dev)
            fresh = focus_mask(images, cut, block=block, mask=mask)
            assert torch.equal(det.mask, fresh.mask) and torch.equal(det.counts, fresh.counts) and torch.equal(words(det.statistics), words(fresh.statistics))
            assert torch.equal(words(whole), words(focus_statistics(images, pooled=True)))
        tissue = None if mask is None else tissue_mask(b)[0].cpu().numpy()
        assert torch.equal(words(det.statistics), fn.as_torch(fn.statistics(fn.tiles_u8()[:2], block, tissue)))
        assert not torch.equal(fresh.mask, focus_mask(a, cut, block=block, mask=mask).mask)


# ------------------------------------------------------------------ 7. cells_mask and focus_mask
@pytest.mark.parametrize("block", fn.BLOCKS[1:], ids=str)
def test_cells_mask_is_repeat_and_crop(dev, block):
    rng = np.random.default_rng(3)
    for n, h, w in (fn.MAIN_SHAPE, (2, 64, 128), (2, 5, 4)):
        gh, gw = -(-h // block[0]), -(-w // block[1])
        cells = (rng.random((n, gh, gw)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (n, gh, gw), dtype=np.uint8)
        tissue = (rng.random((n, h, w)) < 0.7).astype(np.uint8) * 255
        for given in (None, tissue):
            want = torch.from_numpy(fn.cells_mask(cells, h, w, block, given))
            for view in ("dense", "unaligned", "bool"):
                m = None if given is None else on(dev, given)
                if view == "unaligned" and m is not None:
                    m = unaligned_copy(m)
                c = on(dev, cells)
                got, counts = cells_mask(c != 0 if view == "bool" else c, h, w, block, mask=m != 0 if (view == "bool" and m is not None) else m)
                assert got.dtype == torch.uint8 and got.shape == (n, h, w) and counts.dtype == torch.int64 and counts.shape == (n,) and got.device == counts.device == c.device
                assert torch.equal(got.cpu(), want), (n, h, w, view, given is None)
                assert torch.equal(counts.cpu(), want.sum(dim=(1, 2), dtype=torch.int64)), (n, h, w, view, given is None)
    empty, none = cells_mask(torch.empty((0, 1, 1), dtype=torch.uint8, device=dev), 5, 7, block)
    assert empty.shape == (0, 5, 7) and none.shape == (0,)


def test_focus_mask_is_its_steps(dev):
    sharp = fn.real_crop()
    images = np.concatenate([sharp, fn.box_blur(sharp, 3)])      # three tiles and their blurred twins
    x = on(dev, images)
    n, h, w = 6, 150, 203
    for block, mask, min_pixels in (((64, 64), None, None), ((32, 32), "luminosity", None), ((16, 64), "tissue", 100), ((128, 64), None, 0)):
        tissue = tissue_mask(x)[0] if mask is not None else None
        given = tissue if mask == "tissue" else mask
        det = focus_mask(x, 400.0, block=block, mask=given, min_pixels=min_pixels)
        assert isinstance(det, FocusDetection) and det.mask.dtype == torch.uint8 and det.mask.shape == (n, h, w) and det.counts.dtype == torch.int64 and det.counts.shape == (n,)
        stats = focus_statistics(x, block=block, mask=given)
        assert torch.equal(words(det.statistics), words(stats))
        assert torch.equal(words(stats), fn.as_torch(fn.statistics(images, block, None if tissue is None else tissue.cpu().numpy())))
        cells = stats.sharp(400.0, min_pixels=(block[0] * block[1]) // 4 if min_pixels is None else min_pixels)
        out, counts = cells_mask(cells, h, w, block, mask=tissue)
        assert torch.equal(det.mask, out) and torch.equal(det.counts, counts) and torch.equal(counts, out.sum(dim=(1, 2), dtype=torch.int64))
        # the cells by the exact rationals: no cell of this input lies within rounding of the threshold
        s = words(stats).numpy()
        exact = np.zeros(s.shape[1:], dtype=np.uint8)
        least = (block[0] * block[1]) // 4 if min_pixels is None else min_pixels
        for index in np.ndindex(exact.shape):
            var = fn.variance_exact(int(s[0][index]), int(s[1][index]), int(s[2][index]))
            assert var is None or abs(float(var) - 400.0) > 1e-6
            exact[index] = var is not None and s[0][index] >= least and var >= 400
        assert torch.equal(cells.cpu(), torch.from_numpy(exact))
        assert torch.equal(det.mask.cpu(), torch.from_numpy(fn.cells_mask(exact, h, w, block, None if tissue is None else tissue.cpu().numpy())))
    det = focus_mask(x, 400.0)
    assert int(det.counts[:3].sum()) > 4 * int(det.counts[3:].sum())      # the blurred twins lose most of their cells
    nhwc = focus_mask(x.permute(0, 2, 3, 1).contiguous(), 400.0, channel_axis=-1)
    assert torch.equal(nhwc.mask, det.mask) and torch.equal(nhwc.counts, det.counts)


def test_focus_mask_feeds_the_masked_calls(dev):
    x = on(dev, fn.real_crop())
    det = focus_mask(x, 400.0, block=(32, 32), mask="luminosity")
    assert 0 < int(det.counts.sum()) < det.mask.numel()
    norm = Macenko(device=dev, backend="torch_hip")
    norm.fit(synth.reference_tile(128, 128).to(dev))
    out = norm.transform(x, mask=det.mask)
    outside = (det.mask == 0)[:, None].expand_as(x)
    assert out.shape == x.shape and torch.equal(out[outside].to(torch.float32), x[outside].to(torch.float32))      # the masked-out pixels are copied


# ------------------------------------------------------------------ 8. the raw C ABI: a refusal returns its code and leaves the output untouched
def test_raw_abi_refusals_leave_the_output_untouched(dev):
    lib = _native.require()
    BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
    x, mask = on(dev, fn.tiles_u8()), on(dev, fn.tiles_mask())
    n, h, w = fn.MAIN_SHAPE
    stream = _native.stream_ptr(dev)
    out = torch.full((4 * n * 19 * 26,), POISON, dtype=torch.int64, device=dev)      # room for the (8, 8) grid
    levels = torch.full((n, h, w), 171, dtype=torch.uint8, device=dev)
    counts = torch.full((n,), POISON, dtype=torch.int64, device=dev)
    cells = torch.ones((n, 3, 4), dtype=torch.uint8, device=dev)
    u8 = _native.DTYPE_CODES[torch.uint8]

    def stat(images=x.data_ptr(), dtype=u8, n_=n, h_=h, w_=w, bh=0, bw=0, pooled=0, o=out.data_ptr()):
        return lib.sx_focus_statistics(images, dtype, n_, h_, w_, 0, bh, bw, pooled, o, stream)

    def mstat(images=x.data_ptr(), dtype=u8, n_=n, h_=h, w_=w, bh=0, bw=0, pooled=0, m=mask.data_ptr(), o=out.data_ptr()):
        return lib.sx_focus_statistics_masked(images, dtype, n_, h_, w_, 0, bh, bw, pooled, m, o, stream)

    for call in (stat, mstat):
        assert call(images=None) == BAD and call(o=None) == BAD
        assert call(n_=0) == BAD and call(h_=-1) == BAD and call(w_=0) == BAD
        for bh, bw in ((7, 8), (8, 12), (0, 64), (64, 0), (96, 64), (64, 100), (-8, 8)):
            assert call(bh=bh, bw=bw) == BAD and "block sides must each be 8, 16, 32, 64 or a multiple of 64" in _native.last_error(lib), (bh, bw)
        assert call(bh=64, bw=64, pooled=1) == BAD and "pooled" in _native.last_error(lib)
        assert call(dtype=17) == DTYPE and call(dtype=17, bh=128, bw=128) == DTYPE
    assert mstat(m=None) == BAD and "mask pointer is null" in _native.last_error(lib)
    assert lib.sx_grey_map(None, u8, n, h, w, 0, levels.data_ptr(), stream) == BAD and lib.sx_grey_map(x.data_ptr(), u8, n, h, w, 0, None, stream) == BAD
    assert lib.sx_grey_map(x.data_ptr(), u8, n, 0, w, 0, levels.data_ptr(), stream) == BAD and lib.sx_grey_map(x.data_ptr(), 9, n, h, w, 0, levels.data_ptr(), stream) == DTYPE

    def cmask(c=cells.data_ptr(), n_=n, h_=h, w_=w, bh=64, bw=64, o=levels.data_ptr(), k=counts.data_ptr()):
        return lib.sx_cells_mask(c, n_, h_, w_, bh, bw, None, o, k, stream)

    assert cmask(c=None) == BAD and cmask(o=None, k=None) == BAD and cmask(n_=0) == BAD and cmask(h_=0) == BAD and cmask(w_=-3) == BAD
    for bh, bw in ((0, 0), (7, 8), (64, 100), (48, 64)):
        assert cmask(bh=bh, bw=bw) == BAD and "block sides" in _native.last_error(lib), (bh, bw)
    torch.cuda.synchronize(dev)
    assert bool((out == POISON).all()) and bool((levels == 171).all()) and bool((counts == POISON).all())
    # and the calls as they should be, on the same buffers: the mask alone, the counts alone
    assert cmask() == 0 and bool((levels == 1).all()) and counts.tolist() == [h * w] * n
    only = torch.full((n,), POISON, dtype=torch.int64, device=dev)
    assert cmask(o=None, k=only.data_ptr()) == 0 and only.tolist() == [h * w] * n
    assert stat(bh=8, bw=8) == 0 and torch.equal(out.cpu().view(4, n, 19, 26), fn.as_torch(fn.want(fn.MAIN_SHAPE, (8, 8))))
