"""Saturation-channel tissue detection on the GPU, every result an integer and every check exact (torch.equal with the numpy restatements of
tests/_saturation_numpy.py, which the CPU tests pin to exact rationals and to scipy): the saturation map over element types and layouts;
the median filter for every size on a shape of two full 64 x 64 blocks and a ragged remainder both ways; the level histogram and
threshold; saturation_mask against its own steps; and a captured graph that reads the image at replay."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import (LevelHistogram, Macenko, SaturationDetection, _native, level_histogram, level_mask, median_filter, otsu_level, refine_mask, saturation_map,
                        saturation_mask, synth)
from tests import _masked_numpy as mn
from tests import _saturation_numpy as sn
from tests.conftest import TORCH_DTYPES
from tests.test_tissue_mask_gpu import unaligned_copy

pytestmark = pytest.mark.gpu

LAYOUTS = ("nchw", "nhwc", "unaligned")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def in_layout(x: torch.Tensor, layout: str) -> tuple[torch.Tensor, int]:
    if layout == "nhwc":
        return x.permute(0, 2, 3, 1).contiguous(), -1
    return (unaligned_copy(x) if layout == "unaligned" else x), 1


def assert_map(x_cpu: torch.Tensor, dev, what) -> None:
    """saturation_map of x in every layout equals the restatement on the same stored elements."""
    want = torch.from_numpy(sn.saturation_map(sn.as_numpy(x_cpu)))
    for layout in LAYOUTS:
        x, axis = in_layout(x_cpu.to(dev), layout)
        got = saturation_map(x, channel_axis=axis)
        assert got.dtype == torch.uint8 and got.shape == want.shape and got.device == x.device, (what, layout)
        assert torch.equal(got.cpu(), want), (what, layout)


# ------------------------------------------------------------------ 1. the saturation map
@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_saturation_map_dtypes_layouts_shapes(dev, name):
    dt = TORCH_DTYPES[name]
    for kind in ("he", "noise"):
        for index in range(len(sn.MAP_SHAPES)):
            assert_map(synth.as_dtype(sn.map_tiles_u8(kind, index), dt), dev, (kind, index, name))


@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_saturation_map_full_ladder(dev, name):
    ladder = sn.ladder_u8()
    assert_map(synth.as_dtype(ladder, TORCH_DTYPES[name]), dev, name)
    if name in ("u8", "f32", "f64"):      # the ladder's own values: S = 255 for m = 0 (M > 0), 0 for m = M
        got = saturation_map(synth.as_dtype(ladder, TORCH_DTYPES[name]).to(dev))[0].cpu()
        assert got[0].tolist() == [0] + [255] * 255 and got[1].tolist() == [0] * 256
        assert got[2].tolist() == [0, 255] + [(510 + M) // (2 * M) for M in range(2, 256)]


@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "f64"])
def test_saturation_map_special_floats(dev, name):
    x = sn.special_floats(TORCH_DTYPES[name])
    assert_map(x, dev, name)
    got = saturation_map(x.to(dev))[0].cpu()
    assert got[0, 0].item() == 0 and got[0, 5].item() == 0      # a NaN in one channel, or in all: S = 0
    assert got[0, 1].item() == 255 and got[0, 2].item() == 255 and got[0, 3].item() == 255 and got[0, 4].item() == 255      # +-inf and out-of-range values clamp


def test_unit_floats_give_the_uint8_map(dev):
    for kind in ("he", "noise"):
        u8 = sn.map_tiles_u8(kind, 1)
        want = saturation_map(u8.to(dev))
        for dt in (torch.float32, torch.float64):
            assert torch.equal(saturation_map((u8.to(torch.float32) / 255.0).to(dt).to(dev)), want), (kind, dt)
            assert torch.equal(saturation_map((u8.to(torch.float64) / 255.0).to(dt).to(dev)), want), (kind, dt)


# ------------------------------------------------------------------ 2. the median filter
@pytest.mark.parametrize("size", sn.SIZES)
def test_median_every_generator_on_the_main_shape(dev, size):
    assert sn.MAIN_SHAPE[1] > 2 * sn.BLOCK[0] and sn.MAIN_SHAPE[1] % sn.BLOCK[0] and sn.MAIN_SHAPE[2] > 2 * sn.BLOCK[1] and sn.MAIN_SHAPE[2] % sn.BLOCK[1] and sn.MAIN_SHAPE[2] % 4
    for name in sn.GENERATORS:
        levels = torch.from_numpy(sn.levels_case(name).copy()).to(dev)
        got = median_filter(levels, size)
        assert got.dtype == torch.uint8 and got.shape == levels.shape and got.device == levels.device
        assert torch.equal(got.cpu(), torch.from_numpy(sn.median_case(name, size).copy())), (name, size)
        if name == "mask01":
            assert torch.equal(got.cpu(), torch.from_numpy(sn.majority(sn.levels_case(name), size))), size      # the majority count
            assert torch.equal(median_filter(levels.bool(), size), got), size      # a bool mask is read as 0 / 1
        if name == "constant":
            assert torch.equal(got, levels)


@pytest.mark.parametrize("size", [3, 15])
def test_median_small_shapes_views_and_identities(dev, size):
    for shape in sn.SMALL_SHAPES:
        levels = torch.from_numpy(sn.levels_case("random", shape).copy()).to(dev)
        assert torch.equal(median_filter(levels, size).cpu(), torch.from_numpy(sn.median_case("random", size, shape).copy())), (shape, size)
    levels = torch.from_numpy(sn.levels_case("random").copy()).to(dev)
    want = median_filter(levels, size)
    assert torch.equal(median_filter(255 - levels, size), 255 - want)      # the median commutes with the complement
    assert torch.equal(median_filter(levels[:, None], size), want)      # (N, 1, H, W)
    assert torch.equal(median_filter(unaligned_copy(levels), size), want)
    empty = median_filter(torch.empty((0, 5, 7), dtype=torch.uint8, device=dev), size)
    assert empty.shape == (0, 5, 7) and empty.dtype == torch.uint8
    # tiles never see each other: a tile filtered alone gives the bytes it has in the batch
    assert torch.equal(median_filter(levels[1:2].contiguous(), size), want[1:2])


# ------------------------------------------------------------------ 3. histogram and threshold of a level map
def test_level_histogram_is_bincount(dev):
    for name in ("random", "real", "constant", "mask01"):      # (constant: every lane hits one bin)
        levels_np = sn.levels_case(name)
        want = torch.from_numpy(sn.histogram(levels_np))
        for view in ("dense", "unaligned", "n1hw", "vec4"):
            levels = torch.from_numpy(levels_np.copy()).to(dev)
            expect = want
            if view == "unaligned":
                levels = unaligned_copy(levels)
            elif view == "n1hw":
                levels = levels[:, None]
            elif view == "vec4":      # (H * W a multiple of 4: the vectorised loads)
                levels, expect = levels[:, :, :200].contiguous(), torch.from_numpy(sn.histogram(levels_np[:, :, :200]))
            hist = level_histogram(levels)
            assert isinstance(hist, LevelHistogram) and hist.counts.dtype == torch.int64 and hist.counts.shape == (levels.shape[0], 256) and hist.counts.device == levels.device
            assert torch.equal(hist.counts.cpu(), expect), (name, view)
            assert hist.pixels.dtype == torch.int64 and torch.equal(hist.pixels.cpu(), expect.sum(dim=1)), (name, view)
            pooled = level_histogram(levels, pooled=True)
            assert pooled.counts.shape == (1, 256) and torch.equal(pooled.counts.cpu()[0], expect.sum(dim=0)) and pooled.pixels.item() == int(expect.sum()), (name, view)
            assert torch.equal(LevelHistogram.pool(hist).counts, pooled.counts)


def test_level_mask_thresholds_and_counts(dev):
    levels_np = np.concatenate([sn.levels_case("random"), sn.levels_case("real")[:2]])      # five tiles
    levels_np[4, 0, :4] = (0, 7, 8, 255)
    thresholds = [-1, 0, 7, 254, 255]
    want = torch.from_numpy(sn.mask(levels_np, thresholds))
    assert want[0].all() and not want[4].any()      # a negative threshold sets the tile, 255 clears it
    levels = torch.from_numpy(levels_np).to(dev)
    for cuts in (torch.tensor(thresholds), torch.tensor(thresholds, dtype=torch.int32, device=dev), torch.tensor(thresholds, dtype=torch.int64, device=dev)):
        for view in ("dense", "unaligned", "vec4"):
            src, expect = levels, want
            if view == "unaligned":
                src = unaligned_copy(levels)
            elif view == "vec4":
                src, expect = levels[:, :, :200].contiguous(), want[:, :, :200]
            mask, counts = level_mask(src, cuts)
            assert mask.dtype == torch.uint8 and counts.dtype == torch.int64 and counts.shape == (5,) and mask.device == counts.device == levels.device
            assert torch.equal(mask.cpu(), expect), view
            assert torch.equal(counts.cpu(), expect.sum(dim=(1, 2), dtype=torch.int64)), view
    # every accepted integer dtype, on either device, means its own values: nothing is clamped or cast in the narrow type
    for dtype, values in ((torch.uint8, [0, 5, 7, 254, 255]), (torch.int8, [-1, 0, 7, 127, -128]), (torch.int16, [-300, 0, 7, 254, 300]),
                          (torch.int32, [-(1 << 30), 5, 100, 255, 1 << 30]), (torch.int64, [-(1 << 40), 5, 100, 255, 1 << 40])):
        expect = torch.from_numpy(sn.mask(levels_np, values))
        for where in ("cpu", dev):
            mask, counts = level_mask(levels, torch.tensor(values, dtype=dtype, device=where))
            assert torch.equal(mask.cpu(), expect), (dtype, where)
            assert torch.equal(counts.cpu(), expect.sum(dim=(1, 2), dtype=torch.int64)), (dtype, where)
    for bad in (torch.tensor([1.0] * 5), torch.tensor([True] * 5), torch.tensor([1, 2, 3]), torch.tensor([[1, 2, 3, 4, 5]]), [1, 2, 3, 4, 5], 8.0, True, None):
        with pytest.raises(ValueError, match="thresholds"):
            level_mask(levels, bad)
    mask, counts = level_mask(levels, 7)
    assert torch.equal(mask.cpu(), torch.from_numpy(sn.mask(levels_np, [7] * 5))) and torch.equal(counts, mask.sum(dim=(1, 2), dtype=torch.int64))
    assert level_mask(levels, -5)[0].all() and not level_mask(levels, 1000)[0].any()


def test_level_mask_raw_abi_reads_device_thresholds(dev):
    lib = _native.require()
    levels_np = sn.levels_case("random")
    levels = torch.from_numpy(levels_np.copy()).to(dev)
    n, h, w = levels.shape
    cuts = torch.tensor([-1, 100, 255], dtype=torch.int32, device=dev)
    mask = torch.empty_like(levels)
    counts = torch.full((n,), -1, dtype=torch.int64, device=dev)
    stream = _native.stream_ptr(dev)
    assert lib.sx_level_mask_tiles(levels.data_ptr(), n, h, w, cuts.data_ptr(), mask.data_ptr(), counts.data_ptr(), stream) == 0
    want = torch.from_numpy(sn.mask(levels_np, [-1, 100, 255]))
    assert torch.equal(mask.cpu(), want) and torch.equal(counts.cpu(), want.sum(dim=(1, 2), dtype=torch.int64))
    # counts alone, and the mask alone
    only = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert lib.sx_level_mask_tiles(levels.data_ptr(), n, h, w, cuts.data_ptr(), None, only.data_ptr(), stream) == 0 and torch.equal(only, counts)
    alone = torch.empty_like(levels)
    assert lib.sx_level_mask_tiles(levels.data_ptr(), n, h, w, cuts.data_ptr(), alone.data_ptr(), None, stream) == 0 and torch.equal(alone, mask)
    # the median at the ABI, and its refusal to run in place
    out = torch.empty_like(levels)
    assert lib.sx_median_filter_u8(levels.data_ptr(), out.data_ptr(), n, h, w, 5, stream) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(sn.median_case("random", 5).copy()))
    assert lib.sx_median_filter_u8(levels.data_ptr(), levels.data_ptr(), n, h, w, 5, stream) == _native.SX_ERR_BAD_ARG


# ------------------------------------------------------------------ 4. the pipeline
@pytest.fixture(scope="module")
def real_tiles(dev):
    images, _ = mn.real_images()
    return images[:3, :, 256:406, 128:331].contiguous().to(dev)      # (3, 3, 150, 203): tissue and glass


def test_saturation_mask_is_its_steps(dev, real_tiles):
    x = real_tiles
    levels = median_filter(saturation_map(x), 7)
    assert torch.equal(saturation_map(x).cpu(), torch.from_numpy(sn.saturation_map(x.cpu().numpy())))
    for pooled in (False, True):
        det = saturation_mask(x, pooled=pooled)
        assert isinstance(det, SaturationDetection) and det.mask.dtype == torch.uint8 and det.mask.shape == (3, 150, 203) and det.mask.device == x.device
        assert det.counts.dtype == torch.int64 and det.thresholds.dtype == torch.int64 and det.thresholds.device.type == "cpu" and det.thresholds.shape == (3,)
        cuts = otsu_level(level_histogram(levels, pooled=pooled))
        assert torch.equal(det.thresholds, cuts.repeat(3) if pooled else cuts)
        mask, counts = level_mask(levels, det.thresholds)
        assert torch.equal(det.mask, mask) and torch.equal(det.counts, counts) and torch.equal(counts, mask.sum(dim=(1, 2), dtype=torch.int64))
        assert torch.equal(det.mask.cpu(), torch.from_numpy(sn.mask(levels.cpu().numpy(), det.thresholds.tolist())))
    det = saturation_mask(x, threshold=8)
    assert det.thresholds.tolist() == [8, 8, 8] and torch.equal(det.mask, level_mask(levels, 8)[0]) and torch.equal(det.counts, level_mask(levels, 8)[1])
    raw = saturation_mask(x, threshold=8, median_size=0)
    assert torch.equal(raw.mask, level_mask(saturation_map(x), 8)[0])
    for size in (3, 15):
        assert torch.equal(saturation_mask(x, threshold=8, median_size=size).mask, level_mask(median_filter(saturation_map(x), size), 8)[0])
    nhwc = saturation_mask(x.permute(0, 2, 3, 1).contiguous(), threshold=8, channel_axis=-1)
    assert torch.equal(nhwc.mask, det.mask)
    refined = saturation_mask(x, threshold=8, close_radius=4, element="square", min_object_area=16, min_hole_area=16)
    mask, counts = refine_mask(det.mask, close_radius=4, element="square", min_object_area=16, min_hole_area=16)
    assert torch.equal(refined.mask, mask) and torch.equal(refined.counts, counts) and refined.thresholds.tolist() == [8, 8, 8]
    empty = saturation_mask(torch.empty((0, 3, 5, 7), dtype=torch.uint8, device=dev), threshold=8)
    assert empty.mask.shape == (0, 5, 7) and empty.counts.shape == (0,) and empty.thresholds.shape == (0,)


def test_detected_mask_feeds_macenko(dev, real_tiles):
    x = real_tiles
    det = saturation_mask(x, threshold=8, close_radius=2)
    assert 0 < int(det.counts.sum()) < det.mask.numel()
    norm = Macenko(device=dev, backend="torch_hip")
    norm.fit(synth.reference_tile(128, 128).to(dev))
    out = norm.transform(x, mask=det.mask)
    assert out.shape == x.shape
    outside = (det.mask == 0)[:, None].expand_as(x)
    assert torch.equal(out[outside].to(torch.float32), x[outside].to(torch.float32))      # the masked-out pixels are copied


# ------------------------------------------------------------------ 5. one captured graph
def test_captured_graph_reads_the_image_at_replay(dev):
    a = synth.he_batch(2, 70, 90, seed0=7, scale_step=0.1).to(dev)
    b = synth.background_stripes(synth.he_batch(2, 70, 90, seed0=90, scale_step=0.2)).to(dev)
    x = a.clone()
    saturation_mask(x, threshold=8, median_size=7)      # (warm-up: the library is loaded and every kernel has run once)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture on one stream; a call that synchronised would fail it
        det = saturation_mask(x, threshold=8, median_size=7)
    x.copy_(b)
    graph.replay()
    torch.cuda.synchronize(dev)
    fresh = saturation_mask(b, threshold=8, median_size=7)
    assert torch.equal(det.mask, fresh.mask) and torch.equal(det.counts, fresh.counts) and det.thresholds.tolist() == [8, 8]
    assert not torch.equal(fresh.mask, saturation_mask(a, threshold=8, median_size=7).mask)
