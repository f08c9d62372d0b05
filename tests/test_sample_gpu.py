"""Tissue pixel sampling on the GPU (include/stainx_hip.h: sx_sample_pixels): every output BIT FOR BIT against the numpy restatement of the
rule (tests/_sample_numpy.py) -- ``pixels`` compared as integers of the element's width, ``valid``, ``taken``, ``population`` -- over shapes from
one pixel to several 4096-byte chunks with a ragged end, sample sizes on both sides of the populations, masks that are empty, sparse,
dense, in runs that straddle waves, and exact at K - 1, K, K + 1; pooled groups with empty tiles; the offsets; the five element types with
NaN payloads, infinities and -0.0; both layouts; the rule as a mask; the C ABI's refusals; a captured call replayed on new contents; and
the sample as a batch that the existing masked estimates of Macenko, Reinhard and the luminosity standardiser accept."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import LuminosityStandardizer, Macenko, PixelSample, Reinhard, _native, otsu_mask, sample_pixels, tissue_mask
from tests import _luminosity_numpy as ln
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn
from tests import _sample_numpy as sn
from tests.conftest import TORCH_DTYPES
from tests.test_macenko_mask_gpu import HE_ATOL, MAXC_RTOL      # the bounds of the masked Macenko estimate against its restatement

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 4), (2, 33, 47), (3, 64, 67), (2, 150, 203)]      # (2, 150, 203): eight 4096-byte chunks a tile, the last ragged; 203 is no multiple of 4 or 64
SIZES = [(1, 1), (1, 7), (8, 8), (64, 64)]                                    # (64, 64): n < K for all but the last two shapes
BIG = (1 << 40) + 3
INTS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SET_BYTES = np.array([1, 2, 255], dtype=np.uint8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def as_ints(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(INTS[t.element_size()])


def images_for(shape, name: str, seed: int = 0) -> torch.Tensor:
    """(N, 3, H, W) of the element type, every pixel its own value as far as the type allows."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 * seed + n * h * w)
    if name == "u8":
        return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=g)
    return (torch.rand((n, 3, h, w), dtype=torch.float64, generator=g) * 2.0 - 0.5).to(TORCH_DTYPES[name])


def dress(bits: np.ndarray, seed: int) -> np.ndarray:
    """A 0 / 1 mask with its set bytes drawn from {1, 2, 255}."""
    rng = np.random.default_rng(seed)
    return np.where(bits != 0, SET_BYTES[rng.integers(0, 3, size=bits.shape)], 0).astype(np.uint8)


def exact_mask(shape, count: int, pooled: bool, seed: int) -> np.ndarray | None:
    """Exactly ``count`` set pixels in every group (pooled: in the batch, tile 0 first), or None where a group is smaller than that."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    size = n * h * w if pooled else h * w
    if count < 0 or count > size:
        return None
    rows = []
    for _ in range(1 if pooled else n):
        row = np.zeros(size, dtype=np.uint8)
        row[rng.choice(size, size=count, replace=False)] = 1
        rows.append(row)
    return dress(np.concatenate(rows).reshape(n, h, w), seed)


def masks_for(shape, k: int, pooled: bool) -> dict[str, np.ndarray | None]:
    n, h, w = shape
    rng = np.random.default_rng(n * h * w + k)
    last_only = np.zeros((n, h, w), dtype=np.uint8)
    last_only[-1, -1, -1] = 255
    runs = np.zeros((n, h * w), dtype=np.uint8)      # runs of 63 and 65 set pixels, one unset pixel between them: they straddle the 64-lane and 16-byte boundaries
    pos, length = 3, 63
    while pos < h * w:
        runs[:, pos:pos + length] = 1
        pos += length + 1
        length = 128 - length
    out = {"none": None, "zero": np.zeros((n, h, w), dtype=np.uint8), "last pixel": last_only, "half": dress(rng.random((n, h, w)) < 0.5, 1),
           "hundredth": dress(rng.random((n, h, w)) < 0.01, 2), "runs": dress(runs.reshape(n, h, w), 3)}
    for name, count in (("n == K", k), ("n == K + 1", k + 1), ("n == K - 1", k - 1)):
        m = exact_mask(shape, count, pooled, 4 + count)
        if m is not None:
            out[name] = m
    return out


def check(got: PixelSample, x: torch.Tensor, size, mask: np.ndarray | None, pooled: bool, offset: int, what) -> np.ndarray:
    """Every output against the restatement, bit for bit; returns the restated populations."""
    h, w = size
    pixels, valid, taken, population = sn.sample_pixels(as_ints(x).numpy(), size, mask, pooled, offset)
    groups = 1 if pooled else x.shape[0]
    assert got.pixels.shape == (groups, 3, h, w) and got.pixels.dtype == x.dtype and got.pixels.is_contiguous(), what
    assert got.valid.shape == (groups, h, w) and got.valid.dtype == torch.uint8 and got.taken.shape == (groups,) and got.taken.dtype == torch.int32, what
    assert got.population.shape == (groups,) and got.population.dtype == torch.int64, what
    assert torch.equal(got.population.cpu(), torch.from_numpy(population)), (what, got.population.tolist(), population.tolist())
    assert torch.equal(got.taken.cpu(), torch.from_numpy(taken)), (what, got.taken.tolist(), taken.tolist())
    assert torch.equal(got.valid.cpu(), torch.from_numpy(valid)), what
    assert torch.equal(as_ints(got.pixels).cpu(), torch.from_numpy(pixels)), what
    return population


def offsets_for(mask: np.ndarray | None, shape, pooled: bool) -> list[int]:
    n, h, w = shape
    counts = np.full(n, h * w) if mask is None else (mask.reshape(n, -1) != 0).sum(axis=1)
    smallest = int(counts.sum()) if pooled else int(counts.min())
    return sorted({0, 1, max(smallest - 1, 0), BIG})


# ------------------------------------------------------------------------------------------------ 1. the rule, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_for_bit_against_the_restatement(dev, shape):
    x = images_for(shape, "u8")
    xd = x.to(dev)
    seen = set()
    for size in SIZES:
        k = size[0] * size[1]
        for pooled in (False, True):
            for name, mask in masks_for(shape, k, pooled).items():
                md = None if mask is None else torch.from_numpy(mask).to(dev)
                every = name in ("none", "half")      # every offset where most groups are larger than K; the ends of the range elsewhere
                for offset in offsets_for(mask, shape, pooled) if every else (0, BIG):
                    population = check(sample_pixels(xd, size, mask=md, pooled=pooled, offset=offset), x, size, mask, pooled, offset, (shape, size, name, pooled, offset))
                    seen |= {"below" if p < k else "equal" if p == k else "above" for p in population.tolist()}
    if shape[1] * shape[2] * shape[0] > 1:
        assert {"below", "above"} <= seen, seen      # (both branches of the rule ran)
    if shape[0] * shape[1] * shape[2] >= 64:
        assert "equal" in seen


def test_size_forms_bool_masks_mask_shapes_and_unaligned_masks(dev):
    shape = (3, 64, 67)
    x = images_for(shape, "u8", 1)
    xd = x.to(dev)
    mask = masks_for(shape, 64, False)["half"]
    md = torch.from_numpy(mask).to(dev)
    want = sample_pixels(xd, (1, 50), mask=md, offset=9)
    check(want, x, (1, 50), mask, False, 9, "reference")
    for what, got in (("int size", sample_pixels(xd, 50, mask=md, offset=9)), ("list size", sample_pixels(xd, [1, 50], mask=md, offset=9)),
                      ("bool mask", sample_pixels(xd, 50, mask=md != 0, offset=9)), ("(N, 1, H, W) mask", sample_pixels(xd, 50, mask=md[:, None], offset=9)),
                      ("CPU images", sample_pixels(x, 50, mask=md, offset=9))):
        assert all(torch.equal(a, b) for a, b in zip(got, want)), what
    # a mask and images that start 1, 5 and 15 bytes behind a 16-byte address: the words that straddle a tile's ends are read byte by byte
    for shift in (1, 5, 15):
        flat = torch.zeros(md.numel() + 16, dtype=torch.uint8, device=dev)
        view = flat[shift:shift + md.numel()].view(md.shape)
        view.copy_(md)
        flat[:shift] = 255      # (what lies outside the mask is set: it must not be counted)
        flat[shift + md.numel():] = 255
        xflat = torch.empty(xd.numel() + 16, dtype=torch.uint8, device=dev)
        xview = xflat[shift:shift + xd.numel()].view(xd.shape)
        xview.copy_(xd)
        assert view.data_ptr() % 16 == shift and view.is_contiguous()
        for pooled in (False, True):
            check(sample_pixels(xview, (8, 8), mask=view, pooled=pooled, offset=3), x, (8, 8), mask, pooled, 3, ("unaligned", shift, pooled))
    # no tiles: empty groups; a pooled call keeps its one row
    none = sample_pixels(xd[:0], (2, 3), mask=md[:0])
    assert none.pixels.shape == (0, 3, 2, 3) and none.valid.shape == (0, 2, 3) and none.taken.shape == (0,) and none.population.shape == (0,)
    none = sample_pixels(xd[:0], (2, 3), pooled=True)
    assert none.pixels.shape == (1, 3, 2, 3) and not none.pixels.any() and not none.valid.any() and none.taken.tolist() == [0] and none.population.tolist() == [0]


# ------------------------------------------------------------------------------------------------ 2. pooled groups
def test_pooled_groups_with_empty_tiles(dev):
    shape = (3, 64, 67)
    x = images_for(shape, "u8", 2)
    xd = x.to(dev)
    mask = masks_for(shape, 64, False)["half"].copy()
    mask[1] = 0      # a tile without a masked-in pixel between two that have some
    for size in ((1, 7), (8, 8), (64, 64), (96, 96)):
        for offset in (0, 1, BIG):
            for pooled in (True, False):
                check(sample_pixels(xd, size, mask=torch.from_numpy(mask).to(dev), pooled=pooled, offset=offset), x, size, mask, pooled, offset, ("middle tile empty", size, offset, pooled))
    got = sample_pixels(xd, (8, 8), mask=torch.zeros((3, 64, 67), dtype=torch.uint8, device=dev), pooled=True)      # a batch with none at all
    assert got.population.tolist() == [0] and got.taken.tolist() == [0] and not got.valid.any() and not got.pixels.any()
    # a pooled one-tile batch is the tile's own row; a tile's row is the same alone and inside a batch
    md = torch.from_numpy(mask).to(dev)
    batch = sample_pixels(xd, (8, 8), mask=md, offset=5)
    for t in range(3):
        for alone in (sample_pixels(xd[t:t + 1], (8, 8), mask=md[t:t + 1], offset=5), sample_pixels(xd[t:t + 1], (8, 8), mask=md[t:t + 1], offset=5, pooled=True)):
            assert all(torch.equal(a, b[t:t + 1]) for a, b in zip(alone, batch)), t


# ------------------------------------------------------------------------------------------------ 3. element types and layouts
SPECIALS = {"f16": (0x7e01, 0x7c00, 0x8000), "bf16": (0x7fc1, 0x7f80, 0x8000), "f32": (0x7fc01234, 0x7f800000, 0x80000000),
            "f64": (0x7ff8000000001234, 0x7ff0000000000000, 0x8000000000000000)}      # a NaN with a payload, +infinity, -0.0


def signed(bits: int, width: int) -> int:
    return bits - (1 << 8 * width) if bits >= 1 << (8 * width - 1) else bits


@pytest.mark.parametrize("name", ["u8", "f16", "bf16", "f32", "f64"])
def test_element_types_special_values_and_layouts(dev, name):
    for shape in ((2, 33, 47), (2, 150, 203)):
        n, h, w = shape
        x = images_for(shape, name, 3)
        mask = masks_for(shape, 64, False)["half"]
        first = np.flatnonzero(mask[0].reshape(-1))[:3]      # the ranks 0, 1, 2 of tile 0 (and of the pooled batch)
        if name != "u8":
            ints = as_ints(x)
            for c in range(3):
                for pixel, bits in zip(first, SPECIALS[name]):
                    ints[0, c].view(-1)[pixel] = signed(bits, x.element_size())
            x = ints.view(x.dtype)
            assert torch.isnan(x[0, 0].view(-1)[first[0]]) and torch.isinf(x[0, 0].view(-1)[first[1]]) and x[0, 0].view(-1)[first[2]] == 0
        xd, md = x.to(dev), torch.from_numpy(mask).to(dev)
        nhwc = xd.permute(0, 2, 3, 1).contiguous()
        for size, offset in (((64, 64), 0), ((8, 8), 0), ((1, 7), BIG)):      # (64, 64) on 33 x 47: n < K, every pixel taken; offset 0: slot 0 holds rank 0
            for pooled in (False, True):
                for m, mnp in ((md, mask), (None, None)):
                    got = sample_pixels(xd, size, mask=m, pooled=pooled, offset=offset)
                    check(got, x, size, mnp, pooled, offset, (name, shape, size, pooled, offset, m is not None))
                    last = sample_pixels(nhwc, size, mask=m, pooled=pooled, offset=offset, channel_axis=-1)
                    assert all(torch.equal(as_ints(a) if a.is_floating_point() else a, as_ints(b) if b.is_floating_point() else b) for a, b in zip(last, got)), (name, shape, size, "NHWC")
                    if name != "u8" and m is not None and offset == 0:
                        slot0 = as_ints(got.pixels)[0, :, 0, 0].tolist()      # rank 0 of tile 0: the NaN, payload and all
                        assert slot0 == [signed(SPECIALS[name][0], x.element_size())] * 3, (name, shape, size, slot0)
                        if size == (64, 64) and shape == (2, 33, 47):
                            flat = as_ints(got.pixels)[0, 0].view(-1)[:3].tolist()
                            assert flat == [signed(b, x.element_size()) for b in SPECIALS[name]], (name, flat)


def test_the_rule_as_a_mask(dev):
    x8 = mn.real_crops(128)[2:5]
    for name in ("u8", "f32"):
        x = (x8 if name == "u8" else x8.float() / 255.0).to(dev)
        for threshold in (0.8, 0.5):
            explicit = tissue_mask(x, threshold)[0]
            for pooled in (False, True):
                got = sample_pixels(x, (16, 16), mask="luminosity", luminosity_threshold=threshold, pooled=pooled, offset=7)
                want = sample_pixels(x, (16, 16), mask=explicit, pooled=pooled, offset=7)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), (name, threshold, pooled)
                check(got, x.cpu(), (16, 16), explicit.cpu().numpy(), pooled, 7, (name, threshold, pooled))
        assert 0 < int(sample_pixels(x, 4, mask="luminosity", pooled=True).population) < x.shape[0] * 128 * 128


# ------------------------------------------------------------------------------------------------ 4. the C ABI and capture
def test_c_abi_refusals_launch_nothing(dev):
    lib = _native.require()
    n, h, w, k = 2, 33, 47, 16
    x = images_for((n, h, w), "u8", 4).to(dev)
    need = lib.sx_sample_workspace_bytes(n, h, w)
    outs = [torch.full((n, 3, k), 7, dtype=torch.uint8, device=dev), torch.full((n, k), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.int32, device=dev),
            torch.full((n,), 7, dtype=torch.int64, device=dev)]
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    before = [t.clone() for t in outs + [ws]]

    def call(size=k, offset=0, pixels=outs[0].data_ptr(), nbytes=need):
        return lib.sx_sample_pixels(x.data_ptr(), 0, n, h, w, 0, None, 0, size, offset, pixels, outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), ws.data_ptr(), nbytes,
                                    _native.stream_ptr(dev))

    for what, rc in (("null output", call(pixels=None)), ("sample_size 0", call(size=0)), ("sample_size 2^24 + 1", call(size=(1 << 24) + 1)), ("short workspace", call(nbytes=need - 1)),
                     ("negative offset", call(offset=-1))):
        assert rc == _native.SX_ERR_BAD_ARG, (what, rc)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs + [ws], before))      # nothing was enqueued
    assert call() == 0, _native.last_error()
    torch.cuda.synchronize()
    got = PixelSample(outs[0].view(n, 3, 1, k), outs[1].view(n, 1, k), outs[2], outs[3])
    check(got, x.cpu(), (1, k), None, False, 0, "raw call")


def test_captured_call_replays_on_new_contents(dev):
    shape = (2, 150, 203)
    a, b = images_for(shape, "f32", 5), images_for(shape, "f32", 6)
    ma, mb = masks_for(shape, 64, True)["half"], masks_for(shape, 64, True)["runs"]
    x, m = a.to(dev), torch.from_numpy(ma).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        sample_pixels(x, (8, 8), mask=m, pooled=True, offset=11)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a single chain: three launches, no parallel branches
        out = sample_pixels(x, (8, 8), mask=m, pooled=True, offset=11)
    graph.replay()
    torch.cuda.synchronize()
    check(out, a, (8, 8), ma, True, 11, "replay, first contents")
    x.copy_(b.to(dev))
    m.copy_(torch.from_numpy(mb).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    check(out, b, (8, 8), mb, True, 11, "replay, new contents")


# ------------------------------------------------------------------------------------------------ 5. the consumers
@pytest.fixture(scope="module")
def slide(dev):
    """Three 96 x 96 crops of the real fixture that hold tissue and glass, each under its Otsu mask, sampled to (64, 64) and concatenated:
    the sample as arrays on the host, and on the device."""
    images, _ = mn.real_images()
    crops = [images[2:3, :, 200:296, 600:696], images[3:4, :, 464:560, 464:560], images[4:5, :, 0:96, 0:96]]
    samples = []
    for i, crop in enumerate(crops):
        x = crop.contiguous().to(dev)
        mask = otsu_mask(x).mask
        s = sample_pixels(x, (64, 64), mask=mask, offset=i)
        check(s, crop.contiguous(), (64, 64), mask.cpu().numpy(), False, i, ("crop", i))
        samples.append(s)
    s = PixelSample.cat(*samples)
    assert s.pixels.shape == (3, 3, 64, 64) and s.pixels.dtype == torch.uint8 and s.valid.shape == (3, 64, 64)
    assert all(0 < int(t) <= 4096 for t in s.taken) and torch.equal(s.valid.flatten(1).sum(1).to(torch.int32), s.taken)
    return s, s.pixels.cpu().numpy(), s.valid.cpu().numpy() != 0


def test_consumer_macenko(dev, slide):
    s, pixels, valid = slide
    got = Macenko(device=dev, mask=None).estimate(s.pixels, pooled=True, mask=s.valid)
    row = mm.estimate(pixels, valid, pooled=True, signs="positive_sum")[0]
    assert row["kept"] >= 3 and row["plane"]
    he, mc = got.stain_matrices.cpu().numpy(), got.max_concentrations.cpu().numpy()
    assert he.shape == (1, 3, 2) and mc.shape == (1, 2)
    print(f"Macenko on the sample: |HE - restated| {np.abs(he[0] - row['he']).max():.2e} (bound {HE_ATOL}), maxC rel {np.abs(mc[0] / row['max_c'] - 1).max():.2e} (bound {MAXC_RTOL})")
    np.testing.assert_allclose(he[0], row["he"], rtol=0, atol=HE_ATOL)
    np.testing.assert_allclose(mc[0], row["max_c"], rtol=MAXC_RTOL, atol=0)


def test_consumer_reinhard(dev, slide):
    s, pixels, valid = slide
    got = Reinhard(device=dev).estimate(s.pixels, pooled=True, mask=s.valid)
    mean, std, count = mn.reinhard_stats(pixels, valid, per_tile=False)
    assert int(count[0]) == int(s.taken.sum())
    print(f"Reinhard on the sample: |mean - restated| {np.abs(got.mean.cpu().numpy() - mean).max():.2e}, |std - restated| {np.abs(got.std.cpu().numpy() - std).max():.2e}")
    np.testing.assert_allclose(got.mean.cpu().numpy(), mean, rtol=0, atol=2e-3)            # tests/test_tissue_mask_gpu.py:138 (LAB units, 0..255)
    np.testing.assert_allclose(got.std.cpu().numpy(), std, rtol=1e-4, atol=1e-3)           # tests/test_tissue_mask_gpu.py:139


def test_consumer_luminosity(dev, slide):
    """The restatement has the rank rule and the float64 luminance; its own GPU test checks the percentile exactly against another kernel and
    has no bound to borrow.  The bound here: an order statistic moves by at most the largest change of any element, and the float32
    luminance of a uint8 pixel -- three table values, each within half an ulp, times three constants, added -- lies within 4 ulp of 1 of the
    float64 one, 2.4e-7; 1e-6 leaves room for the float32 result's own rounding and is a hundredth of the step between two grey levels."""
    s, pixels, valid = slide
    for percentile in (50.0, 95.0):
        got = LuminosityStandardizer(percentile).estimate(s.pixels, pooled=True, mask=s.valid)
        y = np.sort(ln.luminance(pixels)[valid])
        assert got.pixels.tolist() == [y.size] and y.size == int(s.taken.sum())
        want = y[ln.rank(y.size, percentile) - 1]
        print(f"luminosity percentile {percentile} on the sample: |Y_p - restated| {abs(float(got.luminance[0]) - want):.2e} (bound 1e-6)")
        assert abs(float(got.luminance[0]) - want) <= 1e-6
