"""Tissue detection on the GPU, every result an integer and every check exact: the luminosity histogram against the EXISTING rule at all
255 cuts (sum(counts[:k]) is tissue_mask's count at k / 256) and against the oracle's lightness; the rule with a cut per tile against
tissue_mask; otsu_mask against its own steps; binary morphology against the numpy restatement of tests/_tissue_detect_numpy.py (pinned to
scipy in the CPU tests); a captured graph that reads cuts, image and mask at replay; and a Macenko transform under a detected mask."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import (LuminosityHistogram, Macenko, TissueDetection, _native, luminosity_histogram, mask_morphology, otsu_mask, otsu_threshold, refine_mask, synth,
                        tissue_mask)
from tests import _tissue_detect_numpy as td
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


def rule_counts_at_every_cut(x: torch.Tensor, axis: int) -> torch.Tensor:
    """(255, N) int64: row k - 1 is the tissue count per tile of sx_tissue_mask at luminosity_threshold = k / 256 (the counts-only form)."""
    lib = _native.require()
    last = axis == -1
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if last else (x.shape[0], x.shape[2], x.shape[3])
    out = torch.zeros((255, n), dtype=torch.int64, device=x.device)
    code, stream = _native.DTYPE_CODES[x.dtype], _native.stream_ptr(x.device)
    for k in range(1, 256):
        assert lib.sx_tissue_mask(x.data_ptr(), code, n, h, w, int(last), k / 256.0, None, out[k - 1].data_ptr(), stream) == 0
    return out


def assert_histogram_is_the_rule(x: torch.Tensor, axis: int, what) -> LuminosityHistogram:
    n = x.shape[0]
    pixels = x[0].numel() // 3
    hist = luminosity_histogram(x, channel_axis=axis)
    assert isinstance(hist, LuminosityHistogram) and hist.counts.dtype == torch.int64 and hist.counts.shape == (n, 256) and hist.counts.device == x.device
    assert hist.pixels.dtype == torch.int64 and hist.pixels.shape == (n,) and bool((hist.pixels == pixels).all()), what
    assert bool((hist.counts >= 0).all())
    want = rule_counts_at_every_cut(x, axis)
    assert torch.equal(hist.counts.cumsum(dim=1)[:, :255].t().contiguous(), want), what
    pooled = luminosity_histogram(x, pooled=True, channel_axis=axis)
    assert pooled.counts.shape == (1, 256) and torch.equal(pooled.counts[0], hist.counts.sum(dim=0)) and pooled.pixels.item() == n * pixels, what
    return hist


# ------------------------------------------------------------------ 1. the histogram
@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_histogram_is_the_rule_at_every_cut(dev, name):
    dt = TORCH_DTYPES[name]
    for case in td.all_cases():
        src = synth.as_dtype(td.tiles_u8(case), dt).to(dev)
        for layout in LAYOUTS:
            x, axis = in_layout(src, layout)
            assert_histogram_is_the_rule(x, axis, (case, name, layout))


@pytest.mark.parametrize("name", ["f32", "f16", "bf16", "f64"])
def test_histogram_of_nan_and_values_outside_the_unit_range(dev, name):
    dt = TORCH_DTYPES[name]
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(3, 3, 33, 47, generator=gen) * 1.6 - 0.2      # below 0 and above 1
    x[1, :, 5:9] = float("nan")
    x[1, 0, 20, :] = float("nan")      # one channel NaN: the pixel's luminance is NaN
    x[2, :, :4] = float("inf")
    x[2, 1, 10] = -float("inf")
    src = x.to(dt).to(dev)
    for layout in LAYOUTS:
        xl, axis = in_layout(src, layout)
        hist = assert_histogram_is_the_rule(xl, axis, (name, layout))
        nan_pixels = int(torch.isnan(x[1]).any(dim=0).sum())
        assert hist.counts[1, 255].item() >= nan_pixels      # NaN: background at every cut


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_histogram_of_one_constant_tile(dev, name):
    # every lane of every wave adds to the same bin
    x = synth.as_dtype(torch.full((1, 3, 2048, 2048), 200, dtype=torch.uint8), TORCH_DTYPES[name]).to(dev)
    hist = luminosity_histogram(x)
    (filled,) = torch.nonzero(hist.counts[0]).flatten().tolist()
    assert hist.counts[0, filled].item() == 2048 * 2048 == hist.pixels.item()
    assert tissue_mask(x, (filled + 1) / 256.0)[1].item() == 2048 * 2048 and tissue_mask(x, filled / 256.0)[1].item() == 0
    want = td.oracle_bin_of_grey(200)
    assert abs(filled - want) <= 1, (filled, want)      # (the oracle's lightness and the rule's constant round differently: a neighbouring bin at most)


@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_histogram_against_the_oracle(dev, name):
    dt = TORCH_DTYPES[name]
    for case in td.ORACLE_CASES:
        below, near = td.oracle_histogram(case, name)
        x = synth.as_dtype(td.tiles_u8(case), dt).to(dev)
        got = luminosity_histogram(x).counts.cumsum(dim=1)[:, :255].cpu().numpy()
        off = np.abs(got - below)
        print(f"histogram vs oracle {case} {name}: worst |cumsum difference| {off.max()}, oracle pixels near a cut at most {near.max()}, cuts off {(off > 0).sum()}")
        assert (off <= near).all(), (case, name, int((off - near).max()))


# ------------------------------------------------------------------ 2. a cut per tile
def mask_tiles_raw(x: torch.Tensor, cuts: torch.Tensor, last: bool = False, want_mask: bool = True, want_counts: bool = True):
    lib = _native.require()
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if last else (x.shape[0], x.shape[2], x.shape[3])
    mask = torch.full((n, h, w), 7, dtype=torch.uint8, device=x.device)
    counts = torch.full((n,), -1, dtype=torch.int64, device=x.device)
    rc = lib.sx_tissue_mask_tiles(x.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, int(last), cuts.data_ptr(), mask.data_ptr() if want_mask else None,
                                  counts.data_ptr() if want_counts else None, _native.stream_ptr(x.device))
    assert rc == 0, _native.last_error()
    return mask, counts


def y_cuts(thresholds, dev) -> torch.Tensor:
    lib = _native.require()
    return torch.tensor([lib.sx_tissue_y_cut(float(t)) for t in thresholds], dtype=torch.float32).to(dev)


@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_per_tile_cuts(dev, name):
    dt = TORCH_DTYPES[name]
    for case in ("stripes", "noise", "odd_1", "odd_2"):
        src = synth.as_dtype(td.tiles_u8(case), dt).to(dev)
        n = src.shape[0]
        mixed = [(0.8, 0.5, 0.3, 0.95, 0.66, 0.8)[i % 6] for i in range(n)]
        for layout in LAYOUTS:
            x, axis = in_layout(src, layout)
            last = axis == -1
            for t in (0.8, 0.43):      # equal cuts: the bits of tissue_mask
                want_mask, want_counts = tissue_mask(x, t, channel_axis=axis)
                mask, counts = mask_tiles_raw(x, y_cuts([t] * n, dev), last)
                assert torch.equal(mask, want_mask) and torch.equal(counts, want_counts), (case, name, layout, t)
            mask, counts = mask_tiles_raw(x, y_cuts(mixed, dev), last)      # mixed cuts: each tile alone
            for i, t in enumerate(mixed):
                want_mask, want_counts = tissue_mask(x[i:i + 1].contiguous(), t, channel_axis=axis)
                assert torch.equal(mask[i], want_mask[0]) and counts[i].item() == want_counts.item(), (case, name, layout, i)
            only_mask, untouched = mask_tiles_raw(x, y_cuts(mixed, dev), last, want_counts=False)
            untouched_mask, only_counts = mask_tiles_raw(x, y_cuts(mixed, dev), last, want_mask=False)
            assert torch.equal(only_mask, mask) and torch.equal(only_counts, counts) and bool((untouched == -1).all()) and bool((untouched_mask == 7).all())
            if n > 1:      # a NaN cut: an empty tile, its neighbours as before
                cuts = y_cuts(mixed, dev)
                cuts[1] = float("nan")
                nan_mask, nan_counts = mask_tiles_raw(x, cuts, last)
                keep = [i for i in range(n) if i != 1]
                assert nan_counts[1].item() == 0 and not bool(nan_mask[1].any()) and torch.equal(nan_mask[keep], mask[keep]) and torch.equal(nan_counts[keep], counts[keep])


# ------------------------------------------------------------------ 3. otsu_mask
def test_otsu_mask_is_its_steps(dev):
    for name in ("u8", "f32", "bf16"):
        for case in ("stripes", "real_256", "odd_1"):
            src = synth.as_dtype(td.tiles_u8(case), TORCH_DTYPES[name]).to(dev)
            for layout in ("nchw", "nhwc"):
                x, axis = in_layout(src, layout)
                n = x.shape[0]
                for pooled in (False, True):
                    det = otsu_mask(x, pooled=pooled, channel_axis=axis)
                    assert isinstance(det, TissueDetection) and det.mask.dtype == torch.uint8 and det.mask.shape == (n,) + tuple(src.shape[2:]) and det.counts.dtype == torch.int64
                    want_t = otsu_threshold(luminosity_histogram(x, pooled=pooled, channel_axis=axis))
                    assert det.thresholds.dtype == torch.float64 and det.thresholds.device.type == "cpu" and det.thresholds.shape == (n,)
                    assert torch.equal(det.thresholds, want_t.repeat(n) if pooled else want_t)
                    restated = td.otsu_thresholds(luminosity_histogram(x, pooled=pooled, channel_axis=axis).counts.cpu().numpy())
                    np.testing.assert_array_equal(det.thresholds.numpy(), np.repeat(restated, n) if pooled else restated)
                    for i in range(n):
                        m, c = tissue_mask(x[i:i + 1].contiguous(), float(det.thresholds[i]), channel_axis=axis)
                        assert torch.equal(det.mask[i], m[0]) and det.counts[i].item() == c.item(), (name, case, layout, pooled, i)
    # the striped tiles that hold both tissue and glass: the gap between the modes contains 0.8, so Otsu's mask is the fixed rule's
    x = td.tiles_u8("stripes").to(dev)
    det = otsu_mask(x)
    fixed, fixed_counts = tissue_mask(x, 0.8)
    print("otsu thresholds of the striped tiles:", det.thresholds.tolist())
    assert torch.equal(det.mask[1:5], fixed[1:5]) and torch.equal(det.counts[1:5], fixed_counts[1:5])
    # pooling two batches: the threshold of the concatenated batch
    a, b = x[:3].contiguous(), td.tiles_u8("noise")[:2, :, :96, :96].contiguous().to(dev)
    both = LuminosityHistogram.pool(luminosity_histogram(a), luminosity_histogram(b, pooled=True))
    whole = luminosity_histogram(torch.cat([a, b]), pooled=True)
    assert torch.equal(both.counts, whole.counts) and torch.equal(both.pixels, whole.pixels) and torch.equal(otsu_threshold(both), otsu_threshold(whole))
    # a tile of one grey level has no Otsu threshold: the fallback
    flat = torch.full((2, 3, 16, 16), 240, dtype=torch.uint8, device=dev)
    assert otsu_mask(flat, fallback=0.7).thresholds.tolist() == [0.7, 0.7] and otsu_mask(flat, fallback=0.7).counts.tolist() == [0, 0]
    # with radii: refine_mask of the plain result
    plain = otsu_mask(x)
    refined = otsu_mask(x, open_radius=2, close_radius=3, element="square")
    want_mask, want_counts = refine_mask(plain.mask, open_radius=2, close_radius=3, element="square")
    assert torch.equal(refined.mask, want_mask) and torch.equal(refined.counts, want_counts) and torch.equal(refined.thresholds, plain.thresholds)


# ------------------------------------------------------------------ 4. morphology
def morphology_masks(dev) -> list[tuple[str, np.ndarray]]:
    masks = [(f"random_{d}", td.random_mask((2, 150, 200), d, 11 + i)) for i, d in enumerate((0.05, 0.5, 0.95))]
    masks.append(("real_256_rule", tissue_mask(td.tiles_u8("real_256").to(dev), 0.8)[0].cpu().numpy()))
    for i, shape in enumerate(((3, 37, 70), (2, 5, 7), (1, 3, 4), (1, 800, 230))):      # (the last: 3 workgroups of 256 x 64 each way and a remainder)
        masks.append((f"shape_{shape}", td.random_mask(shape, 0.7, 31 + i)))
    values = td.random_mask((2, 41, 67), 0.6, 41) * np.random.default_rng(42).integers(1, 256, (2, 41, 67)).astype(np.uint8)      # set = any non-zero byte
    masks.append(("bytes_1_to_255", values))
    masks.append(("all_255", np.full((1, 20, 70), 255, dtype=np.uint8)))
    ones_zeros = np.zeros((4, 40, 50), dtype=np.uint8)
    ones_zeros[0::2] = 1      # all-ones next to all-zeros: nothing bleeds across tiles
    masks.append(("ones_next_to_zeros", ones_zeros))
    return masks


@pytest.fixture(scope="module")
def masks(dev):
    return morphology_masks(dev)


@pytest.mark.parametrize("radius", [1, 2, 5, td.MAX_RADIUS])
@pytest.mark.parametrize("element", td.ELEMENTS)
def test_morphology_is_the_numpy_restatement(dev, masks, element, radius):
    for what, mask in masks:
        m = torch.from_numpy(mask).to(dev)
        results = {}
        for op in td.OPS:
            want = td.morphology(mask, op, radius, element)
            got, counts = mask_morphology(m, op, radius, element=element)
            assert got.dtype == torch.uint8 and got.shape == m.shape and counts.dtype == torch.int64 and counts.shape == (m.shape[0],)
            got_np = got.cpu().numpy()
            assert set(np.unique(got_np)) <= {0, 1}
            np.testing.assert_array_equal(got_np != 0, want, err_msg=f"{what} {op} {element} {radius}")
            assert torch.equal(counts, got.sum(dim=(1, 2), dtype=torch.int64)), (what, op)
            results[op] = got_np != 0
        set_in = mask != 0
        assert not (results["open"] & ~set_in).any() and not (set_in & ~results["close"]).any(), what      # open <= input <= close
        assert not (results["erode"] & ~results["open"]).any() and not (results["close"] & ~results["dilate"]).any(), what
        if what in ("random_0.5", "shape_(3, 37, 70)"):      # a byte-misaligned view, and the (N, 1, H, W) bool form
            for op in td.OPS:
                want = torch.from_numpy(results[op]).to(dev)
                assert torch.equal(mask_morphology(unaligned_copy(m), op, radius, element=element)[0] != 0, want), (what, op, "unaligned")
                assert torch.equal(mask_morphology((m != 0).unsqueeze(1), op, radius, element=element)[0] != 0, want), (what, op, "bool")
    m = torch.from_numpy(dict(masks)["ones_next_to_zeros"]).to(dev)
    for op in td.OPS:
        got, counts = mask_morphology(m, op, radius, element=element)
        assert torch.equal(got, m) and counts.tolist() == [2000, 0, 2000, 0], op


def test_morphology_specks_and_holes(dev):
    for element in td.ELEMENTS:
        speck = torch.zeros(2, 64, 300, dtype=torch.uint8, device=dev)
        speck[0, 30, 63] = speck[1, 0, 0] = speck[1, 63, 299] = 1      # lone pixels: inside, across a workgroup's edge, in the corners
        speck[0, 10:20, 100:140] = 1
        opened, counts = mask_morphology(speck, "open", 1, element=element)
        block = torch.zeros_like(speck)
        block[0, 10:20, 100:140] = 1
        if element == "disk":      # disk(1) is the plus: the opening of a rectangle by it loses the four corner pixels
            block[0, [10, 10, 19, 19], [100, 139, 100, 139]] = 0
        assert torch.equal(opened, block) and counts.tolist() == [400 - 4 * (element == "disk"), 0], element
        holes = 1 - speck
        holes[0, 10:20, 100:140] = 1
        holes[0, 15, 120] = 0
        closed, counts = mask_morphology(holes, "close", 1, element=element)
        assert bool(closed.all()) and counts.tolist() == [64 * 300] * 2, element
        # refine_mask: the opening, then the closing; radius 0 skips a step
        both, both_counts = refine_mask(speck, open_radius=1, close_radius=2, element=element)
        want = mask_morphology(mask_morphology(speck, "open", 1, element=element)[0], "close", 2, element=element)
        assert torch.equal(both, want[0]) and torch.equal(both_counts, want[1])
        same, same_counts = refine_mask(speck * 255)
        assert torch.equal(same, speck) and torch.equal(same_counts, speck.sum(dim=(1, 2), dtype=torch.int64))
        only_close, _ = refine_mask(holes, close_radius=1, element=element)
        assert torch.equal(only_close, closed)


# ------------------------------------------------------------------ 5. plumbing
def test_tile_cuts_and_morphology_in_a_captured_graph_read_their_inputs_at_replay(dev):
    lib = _native.require()
    first_x = synth.as_dtype(td.tiles_u8("stripes")[:4], torch.float32).to(dev)
    new_x = synth.as_dtype(td.tiles_u8("noise")[:4, :, :96, :96].contiguous(), torch.float32).to(dev)
    first_cuts, new_cuts = y_cuts([0.8, 0.8, 0.8, 0.8], dev), y_cuts([0.5, 0.9, 0.3, 0.7], dev)
    x, cuts = first_x.clone(), first_cuts.clone()
    made = torch.zeros((4, 96, 96), dtype=torch.uint8, device=dev)
    made_counts = torch.zeros((4,), dtype=torch.int64, device=dev)
    out, scratch = torch.zeros_like(made), torch.zeros_like(made)
    out_counts = torch.zeros_like(made_counts)
    f32 = _native.DTYPE_CODES[torch.float32]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: one stream
        assert lib.sx_tissue_mask_tiles(x.data_ptr(), f32, 4, 96, 96, 0, cuts.data_ptr(), made.data_ptr(), made_counts.data_ptr(), _native.stream_ptr(dev)) == 0
        assert lib.sx_mask_morphology(made.data_ptr(), out.data_ptr(), 4, 96, 96, _native.MORPH_OPS["open"], _native.MORPH_ELEMENTS["disk"], 2, scratch.data_ptr(),
                                      out_counts.data_ptr(), _native.stream_ptr(dev)) == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    first_mask, first_counts = tissue_mask(first_x, 0.8)
    first_open = mask_morphology(first_mask, "open", 2)
    assert torch.equal(made, first_mask) and torch.equal(made_counts, first_counts) and torch.equal(out, first_open[0]) and torch.equal(out_counts, first_open[1])
    x.copy_(new_x)
    cuts.copy_(new_cuts)
    graph.replay()
    torch.cuda.synchronize(dev)
    want_mask, want_counts = mask_tiles_raw(new_x, new_cuts)
    want_open = mask_morphology(want_mask, "open", 2)
    assert torch.equal(made, want_mask) and torch.equal(made_counts, want_counts) and torch.equal(out, want_open[0]) and torch.equal(out_counts, want_open[1])
    assert not torch.equal(want_mask, first_mask)


def test_macenko_under_a_detected_mask(dev):
    ref = synth.reference_tile(96, 96).to(dev)
    x = td.tiles_u8("stripes")[1:5].contiguous().to(dev)
    norm = Macenko(device="cuda").fit(ref)
    det = otsu_mask(x, pooled=True, open_radius=2)
    got = norm.transform(x, mask=det.mask)
    threshold = otsu_threshold(luminosity_histogram(x, pooled=True))
    stepwise, _ = mask_morphology(tissue_mask(x, float(threshold[0]))[0], "open", 2)
    assert torch.equal(det.mask, stepwise) and det.thresholds.tolist() == [float(threshold[0])] * 4
    assert torch.equal(got, norm.transform(x, mask=stepwise))
    background = (det.mask == 0).unsqueeze(1).expand_as(x)
    assert torch.equal(got[background], x[background]) and not torch.equal(got, x)
    assert 0 < int(det.counts.sum()) < x[:, 0].numel()
