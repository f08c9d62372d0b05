"""The JPEG round trip on the GPU, through the C ABI (sx_jpeg_roundtrip, sx_jpeg_roundtrip_masked) and through ``jpeg_compress`` /
``JPEGAugment``.  EVERY comparison is ``torch.equal``: there is no tolerance anywhere.

The yardsticks: tests/_jpeg_numpy.py, the rule in numpy int64 (held to Pillow's bytes by tests/test_jpeg_cpu.py), evaluated ONCE per
(tile, quality, subsampling) and shared; the committed Pillow bytes of tests/golden/jpeg_pillow.npz directly, with no restatement in
between; and ``sx_hsv_apply`` -- an existing, tested call -- for the output rule (its identity row returns every uint8 colour exactly) and
for the copy rule (a row with a NaN copies its tile).

The tiles -- 1x1, 1x7, 7x1, 2x2, 3x5, 5x3 (narrow 4:2:0 tiles: chroma replicated, not filtered), 8x8, 9x17, 16x16, 17x9, 33x31 (partial
blocks in each axis, odd sizes), 64x64, 65x130, 144x128 (several regions with ragged edges, chroma halos across region seams) and 129x129
(one past the 128 x 128 region of 4:2:0 in both axes) -- come in batches of four with a different quality per tile in one launch, the
fourth a NaN (a copy)."""
from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from stainx_amd import JPEGAugment, _native, focus_statistics, jpeg_compress, tissue_mask
from tests import _hsv_numpy as hn
from tests import _jpeg_numpy as jn
from tests.test_hsv_gpu import graph_nodes, off_by_one, row_tensor
from tests.test_hsv_gpu import raw as hsv_raw

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (8, 8), (9, 17), (16, 16), (17, 9), (33, 31), (64, 64), (65, 130), (144, 128), (129, 129))
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
SUBS = (0, 2)
SUB_IDS = ["444", "420"]
NAN, INF = float("nan"), float("inf")
QUALITIES = (10.0, 50.0, 95.0, NAN)
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64)
DTYPE_IDS = [str(d).split(".")[-1] for d in DTYPES]
CL, UNIT = _native.MACENKO_CHANNELS_LAST, _native.MACENKO_NORMALIZE_0_1
OUT_FLAG = {torch.bfloat16: _native.MACENKO_OUT_BF16, torch.float16: _native.MACENKO_OUT_F16}
FIXTURE = Path(__file__).resolve().parent / "golden" / "jpeg_pillow.npz"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ the tiles and their references
@lru_cache(maxsize=None)
def tiles_u8(shape: tuple) -> torch.Tensor:
    """(4, 3, H, W) uint8 on the CPU, seeded: noise, a colour ramp with noise, saturated noise (levels 0 and 255 only), noise."""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([40 + 3 * yy + 2 * xx, 200 - 2 * yy + xx, 90 + yy - 3 * xx]).astype(np.float64) + rng.normal(0.0, 12.0, (3, h, w))
    tiles = np.stack([rng.integers(0, 256, (3, h, w)), np.clip(ramp, 0, 255), rng.integers(0, 2, (3, h, w)) * 255, rng.integers(0, 256, (3, h, w))]).astype(np.uint8)
    return torch.from_numpy(tiles)


@lru_cache(maxsize=None)
def reference(shape: tuple, tile: int, quality: float, sub: int) -> torch.Tensor:
    """(3, H, W) uint8: tile ``tile`` of ``tiles_u8`` after the round trip (the tile itself for a quality that copies)."""
    return torch.from_numpy(jn.roundtrip(tiles_u8(shape)[tile:tile + 1].numpy(), [quality], sub)[0])


def reference_rows(shape: tuple, qualities, sub: int) -> torch.Tensor:
    return torch.stack([reference(shape, t, float(q), sub) for t, q in enumerate(qualities)])


def as_dtype(levels: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """uint8 levels as a tile of ``dtype``: level / 255 in float64, rounded to the type (rint(255 x) gives the level back in every type)."""
    return levels if dtype == torch.uint8 else (levels.to(torch.float64) / 255.0).to(dtype)


def out_dtype_of(x: torch.Tensor, flags: int) -> torch.dtype:
    if x.dtype == torch.uint8:
        for dtype, flag in OUT_FLAG.items():
            if flags & flag:
                return dtype
        return torch.float32 if flags & UNIT else torch.uint8
    return x.dtype


def raw(lib, x: torch.Tensor, qualities: torch.Tensor, sub: int, flags: int = 0, mask: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_jpeg_roundtrip / sx_jpeg_roundtrip_masked on the current stream; ``qualities``: (R,) float32 on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype_of(x, flags), device=x.device)
    assert qualities.dtype == torch.float32 and qualities.is_contiguous() and qualities.dim() == 1
    stream = _native.stream_ptr(x.device)
    if mask is None:
        rc = lib.sx_jpeg_roundtrip(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, qualities.data_ptr(), qualities.shape[0], sub, flags, stream)
    else:
        rc = lib.sx_jpeg_roundtrip_masked(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, qualities.data_ptr(), qualities.shape[0], sub, mask.data_ptr(), flags, stream)
    assert rc == 0, _native.last_error(lib)
    return out


def qs(values, dev) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float32, device=dev).reshape(-1)


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def hsv_identity(lib, x: torch.Tensor, flags: int = 0) -> torch.Tensor:
    return hsv_raw(lib, x, row_tensor(hn.IDENTITY, x.device), flags)


def hsv_copy(lib, x: torch.Tensor, flags: int = 0) -> torch.Tensor:
    return hsv_raw(lib, x, row_tensor((NAN, 1.0, 0.0, 1.0, 0.0), x.device), flags)


def output_rule(lib, levels: torch.Tensor, dtype: torch.dtype, unit: bool) -> torch.Tensor:
    """What a tile of ``dtype`` comes out as when its result is ``levels`` (uint8, on the device): sx_hsv_apply's identity row on the uint8
    result under the flags that give the same output element; where no such call exists (a float tile without / 255; float64) the cast."""
    if not unit:
        return levels.to(dtype)      # (an integer up to 255 is exact in every element type)
    if dtype == torch.float64:
        return (levels.cpu().to(torch.float64) / 255.0).to(levels.device)      # (the IEEE quotient: on the device torch multiplies by a reciprocal)
    return hsv_identity(lib, levels, UNIT | OUT_FLAG.get(dtype, 0))


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_quality_rows_against_the_restatement(dev, lib, shape, sub):
    x = tiles_u8(shape)
    xd = x.to(dev)
    want = reference_rows(shape, QUALITIES, sub)
    out = raw(lib, xd, qs(QUALITIES, dev), sub)
    assert out.dtype == torch.uint8
    differing = int((out.cpu() != want).sum())
    print(f"{shape} subsampling {sub}: {differing} differing bytes of {want.numel()}")
    assert torch.equal(out.cpu(), want), (shape, sub, differing)
    assert torch.equal(out[3], xd[3]) and not torch.equal(out[0], xd[0])      # the NaN tile is the input; the others are not
    assert torch.equal(raw(lib, nhwc(xd), qs(QUALITIES, dev), sub, CL).permute(0, 3, 1, 2), out), "NHWC"      # NCHW and NHWC: the same values
    for t in range(4):      # a tile alone gives the bits it has inside the batch
        assert torch.equal(raw(lib, xd[t:t + 1].contiguous(), qs(QUALITIES[t:t + 1], dev), sub), out[t:t + 1]), t
    if shape == (33, 31):      # the table rule's corners: quality 1 (every entry 255), 49 / 50 (the two scale formulas meet), 100 (all ones)
        corners = (1.0, 49.0, 50.0, 100.0)
        got = raw(lib, xd, qs(corners, dev), sub).cpu()
        assert torch.equal(got, reference_rows(shape, corners, sub))
        assert not torch.equal(got[3], x[3])      # quality 100 is not the identity


@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_gpu_bytes_are_pillows_bytes(dev, lib, sub):
    """No restatement in between: the committed Pillow round trips of a 128 x 128 crop of real tissue at quality 50 and 90, and of the
    fixture's eleven seeded shapes at quality 1, 35, 75 and 100."""
    fixture = np.load(FIXTURE)
    real = torch.from_numpy(fixture["in_real"]).unsqueeze(0).expand(2, -1, -1, -1).contiguous().to(dev)
    want = torch.from_numpy(np.stack([fixture[f"out_real_q50_s{sub}"], fixture[f"out_real_q90_s{sub}"]]))
    got = raw(lib, real, qs((50.0, 90.0), dev), sub).cpu()
    print(f"real tissue, subsampling {sub}: {int((got != want).sum())} bytes differ from Pillow's; the round trip moves a byte by "
          f"{float((want[0].int() - real[0].cpu().int()).abs().float().mean()):.2f} (q 50) / {float((want[1].int() - real[1].cpu().int()).abs().float().mean()):.2f} (q 90) levels on average")
    assert torch.equal(got, want)
    for key in fixture.files:
        if key.startswith("in_") and key != "in_real":
            tile = torch.from_numpy(fixture[key]).unsqueeze(0).expand(4, -1, -1, -1).contiguous().to(dev)
            want = torch.from_numpy(np.stack([fixture[f"out_{key[3:]}_q{q}_s{sub}"] for q in (1, 35, 75, 100)]))
            assert torch.equal(raw(lib, tile, qs((1.0, 35.0, 75.0, 100.0), dev), sub).cpu(), want), key


# ------------------------------------------------------------------ element types
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
@pytest.mark.parametrize("shape", [(33, 31), (144, 128)], ids=["33x31", "144x128"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_element_types_follow_the_output_rule(dev, lib, dtype, shape, sub):
    levels = tiles_u8(shape).to(dev)
    quality = qs(QUALITIES, dev)
    result = raw(lib, levels, quality, sub)      # uint8 in, uint8 out: held to the restatement above
    x = as_dtype(levels, dtype)
    copied = torch.zeros(4, dtype=torch.bool, device=dev)
    copied[3] = True
    variants = ((0, False), (UNIT, True)) if dtype != torch.uint8 else ((UNIT, True), (OUT_FLAG[torch.bfloat16], False), (OUT_FLAG[torch.float16], False),
                                                                       (UNIT | OUT_FLAG[torch.bfloat16], True), (UNIT | OUT_FLAG[torch.float16], True))
    for flags, unit in variants:
        out = raw(lib, x, quality, sub, flags)
        assert out.dtype == out_dtype_of(x, flags)
        if dtype == torch.uint8:
            want = hsv_identity(lib, result, flags)      # the output rule of an existing call on the uint8 result, same flags
        else:
            want = output_rule(lib, result, dtype, unit)
        assert torch.equal(out[:3], want[:3]), (dtype, flags)
        assert torch.equal(out[3], hsv_copy(lib, x, flags)[3]), (dtype, flags, "copy")
        assert torch.equal(raw(lib, nhwc(x), quality, sub, flags | CL).permute(0, 3, 1, 2), out), (dtype, flags, "NHWC")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_float_tiles_are_quantised_by_rint(dev, lib, dtype):
    """(level + 0.49) / 255 is the level, (level + 0.51) / 255 the next one; out-of-range values clamp; a NaN channel is level 0."""
    shape = (33, 31)
    levels = tiles_u8(shape)[:3].clamp(max=254)
    quality = qs((10.0, 50.0, 95.0), dev)
    for sub in SUBS:
        low = raw(lib, ((levels.double() + 0.49) / 255.0).to(dtype).to(dev), quality, sub)
        high = raw(lib, ((levels.double() + 0.51) / 255.0).to(dtype).to(dev), quality, sub)
        assert torch.equal(low, raw(lib, levels.to(dev), quality, sub).to(dtype))
        assert torch.equal(high, raw(lib, (levels + 1).to(dev), quality, sub).to(dtype))
        wild = (levels.double() / 255.0).to(dtype)
        tame = levels.clone()
        wild[:, 0, 3, 4], tame[:, 0, 3, 4] = NAN, 0
        wild[:, 1, 20, 30], tame[:, 1, 20, 30] = -7.5, 0
        wild[:, 2, 32, 0], tame[:, 2, 32, 0] = INF, 255
        wild[:, 2, 0, 30], tame[:, 2, 0, 30] = 1.0 + 2.0**-10, 255
        got = raw(lib, wild.to(dev), quality, sub)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, raw(lib, tame.to(dev), quality, sub).to(dtype))
        assert torch.equal(got.cpu().to(torch.uint8), torch.from_numpy(jn.roundtrip(wild.numpy(), [10.0, 50.0, 95.0], sub)))      # (the restatement's levels_of)


# ------------------------------------------------------------------ invariances
@pytest.mark.parametrize("sub", SUBS, ids=SUB_IDS)
def test_one_row_serves_the_batch_and_150_is_100(dev, lib, sub):
    x = tiles_u8((65, 130)).to(dev)
    assert torch.equal(raw(lib, x, qs((35.0,), dev), sub), raw(lib, x, qs((35.0,) * 4, dev), sub))
    assert torch.equal(raw(lib, x, qs((150.0, 100.5, 1e30, 100.0), dev), sub), raw(lib, x, qs((100.0,), dev), sub))
    assert torch.equal(raw(lib, x, qs((35.9, 1.0, 1.99, 49.999), dev), sub), raw(lib, x, qs((35.0, 1.0, 1.0, 49.0), dev), sub))      # (int)quality


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_copied_tiles_are_hsv_applys_copies(dev, lib, dtype):
    for shape in ((33, 31), (144, 128)):
        x = as_dtype(tiles_u8(shape), dtype).to(dev)
        x = torch.cat([x, x[:1]])      # five tiles, five ways to say "leave this tile"
        quality = qs((NAN, INF, 0.0, -3.0, 0.5), dev)
        flag_sets = (0, UNIT) if dtype != torch.uint8 else (0, UNIT, OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16])
        for flags in flag_sets:
            want = hsv_copy(lib, x, flags)
            for sub in SUBS:
                assert torch.equal(raw(lib, x, quality, sub, flags), want), (dtype, shape, flags, sub)
            assert torch.equal(raw(lib, nhwc(x), quality, 2, flags | CL).permute(0, 3, 1, 2), want)
        if dtype == torch.uint8:
            assert torch.equal(raw(lib, x, quality, 2), x)      # uint8 in, uint8 out: the same bytes
            assert torch.equal(raw(lib, x, qs((-INF,), dev), 0), x)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_pointers_one_element_off_give_the_aligned_bits(dev, lib, dtype):
    shape = (144, 128)
    x = as_dtype(tiles_u8(shape), dtype).to(dev)
    quality = qs((NAN, 20.0, 75.0, 95.0), dev)
    mask = (torch.rand(4, *shape, device=dev) < 0.7).to(torch.uint8)
    for sub in SUBS:
        want, want_masked = raw(lib, x, quality, sub), raw(lib, x, quality, sub, mask=mask)
        assert torch.equal(raw(lib, off_by_one(x), quality, sub), want)
        out = off_by_one(torch.empty_like(want))
        assert torch.equal(raw(lib, x, quality, sub, out=out), want)
        assert torch.equal(raw(lib, x, quality, sub, mask=off_by_one(mask)), want_masked)
        assert torch.equal(raw(lib, off_by_one(x), quality, sub, mask=mask), want_masked)
        assert torch.equal(raw(lib, off_by_one(nhwc(x)), quality, sub, CL).permute(0, 3, 1, 2), want)


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("shape", [(5, 3), (33, 31), (65, 130), (144, 128)], ids=["5x3", "33x31", "65x130", "144x128"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_masks(dev, lib, dtype, shape):
    x = as_dtype(tiles_u8(shape), dtype).to(dev)
    quality = qs((10.0, 50.0, 95.0, NAN), dev)
    for sub in SUBS:
        plain = raw(lib, x, quality, sub)
        copied = raw(lib, x, qs((NAN,), dev), sub)
        assert torch.equal(copied, hsv_copy(lib, x))
        assert torch.equal(raw(lib, x, quality, sub, mask=torch.ones(4, *shape, dtype=torch.uint8, device=dev)), plain)
        assert torch.equal(raw(lib, x, quality, sub, mask=torch.zeros(4, *shape, dtype=torch.uint8, device=dev)), copied)
        half = torch.zeros(4, *shape, dtype=torch.uint8, device=dev)      # a half plane: the codec still reads every pixel
        half[:, :, shape[1] // 2:] = 255
        got = raw(lib, x, quality, sub, mask=half)
        inside = half.bool().unsqueeze(1).expand_as(x)
        assert torch.equal(got[~inside], copied[~inside]) and torch.equal(got[inside], plain[inside])      # out: the input's bytes; in: the unmasked call's
        if dtype == torch.uint8:
            assert torch.equal(got[~inside], x[~inside])
        speckle = (torch.rand(4, *shape, device=dev) < 0.6).to(torch.uint8) * 3      # (non-zero = in)
        inside = speckle.bool().unsqueeze(1).expand_as(x)
        for flags in ((0, UNIT) if dtype != torch.uint8 else (0, UNIT, OUT_FLAG[torch.bfloat16])):
            assert torch.equal(raw(lib, x, quality, sub, flags, mask=speckle), torch.where(inside, raw(lib, x, quality, sub, flags), raw(lib, x, qs((NAN,), dev), sub, flags)))


def real_tile() -> torch.Tensor:
    return torch.from_numpy(np.load(FIXTURE)["in_real"])


def test_luminosity_rule_is_the_explicit_tissue_mask(dev):
    x = real_tile().unsqueeze(0).expand(3, -1, -1, -1).contiguous().to(dev)
    quality = qs((20.0, 50.0, 90.0), dev)
    explicit, counts = tissue_mask(x, 0.7)
    assert 0 < int(counts.sum()) < explicit.numel()
    want = jpeg_compress(x, quality, mask=explicit)
    assert torch.equal(jpeg_compress(x, quality, mask="luminosity", luminosity_threshold=0.7), want)
    assert torch.equal(JPEGAugment(mask="luminosity", luminosity_threshold=0.7, normalize_to_0_1=False)(x, quality), want)
    assert torch.equal(JPEGAugment(normalize_to_0_1=False)(x, quality, mask=explicit.unsqueeze(1)), want)
    assert not torch.equal(want, jpeg_compress(x, quality))


# ------------------------------------------------------------------ the module and the functional form
def test_module_and_functional_form(dev, lib):
    x = tiles_u8((65, 130)).to(dev)
    quality = qs((10.0, 50.0, 95.0, NAN), dev)
    want, want_444 = raw(lib, x, quality, 2), raw(lib, x, quality, 0)
    assert torch.equal(jpeg_compress(x, quality), want) and torch.equal(jpeg_compress(x, quality, subsampling="420"), want) and torch.equal(jpeg_compress(x, quality, subsampling=2), want)
    assert torch.equal(jpeg_compress(x, quality, subsampling="444"), want_444) and torch.equal(jpeg_compress(x, quality, subsampling=0), want_444)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        jpeg_compress(x.cpu(), quality)
    aug = JPEGAugment(normalize_to_0_1=False)
    assert torch.equal(aug(x, quality), want) and torch.equal(aug(x, quality.cpu()), want)
    assert torch.equal(JPEGAugment(subsampling="444", normalize_to_0_1=False)(x, quality), want_444)
    assert torch.equal(JPEGAugment()(x, quality), raw(lib, x, quality, 2, UNIT))      # normalize_to_0_1 defaults to True, as HSVAugment's
    assert torch.equal(jpeg_compress(x, quality, out_dtype=torch.bfloat16), raw(lib, x, quality, 2, OUT_FLAG[torch.bfloat16]))
    assert torch.equal(jpeg_compress(nhwc(x), quality, channel_axis=-1), nhwc(want))
    # one quality for the batch: a (1,) row, a () tensor, a Python int
    one = raw(lib, x, qs((50.0,), dev), 2)
    assert torch.equal(jpeg_compress(x, quality[1:2]), one) and torch.equal(jpeg_compress(x, quality[1]), one) and torch.equal(jpeg_compress(x, 50), one) and torch.equal(aug(x, 50), one)
    assert not torch.equal(jpeg_compress(x, 100), x)      # not the identity
    # CHW in, CHW out
    single = aug(x[1], quality[1:2])
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, want[1])
    assert torch.equal(jpeg_compress(x[1], 50), want[1])
    # p = 0: every quality is NaN, the input comes back exactly
    assert torch.equal(JPEGAugment(p=0.0, normalize_to_0_1=False)(x), x)
    # a draw: the qualities sample_rows gives with the same seed, on the device when the generator is there
    for where in ("cpu", dev):
        drawn = JPEGAugment((5, 100), p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5))
        got = drawn(x)
        again = JPEGAugment((5, 100), p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5)).sample_rows(4, dev)
        assert torch.equal(got, raw(lib, x, again.contiguous(), 2))
        left = torch.isnan(again)
        assert torch.equal(got[left], x[left])


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("mask", [None, "luminosity"], ids=["plain", "luminosity"])
def test_a_captured_forward_replays_with_new_qualities_and_images(dev, mask):
    first_x = real_tile().unsqueeze(0).expand(3, -1, -1, -1).contiguous().to(dev)
    second_x = first_x.flip(-1).contiguous()
    first, second = qs((10.0, 50.0, 95.0), dev), qs((75.0, NAN, 30.0), dev)
    aug = JPEGAugment(normalize_to_0_1=False, mask=mask)
    want_first, want_second = aug(first_x, first), aug(second_x, second)
    assert not torch.equal(want_first, want_second)
    x, buf = first_x.clone(), first.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        aug(x, buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = aug(x, buf)
        types, roots, edges = graph_nodes(dev)
    if mask is None:
        assert types == [0], types      # ONE node, a kernel (hipGraphNodeTypeKernel = 0): no memset node (2), no copy (1)
        assert roots == 1 and edges == 0      # a single branch
    else:
        assert types == [0, 0] and roots == 1 and edges == 1, (types, roots, edges)      # the rule's mask launch in front, one chain
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_first)
    buf.copy_(second)
    x.copy_(second_x)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_second)


# ------------------------------------------------------------------ sanity of the effect
def test_quality_orders_the_damage_on_real_tissue(dev):
    """Printed, with a loose guard: the PSNR of a real crop against its round trip falls monotonically over quality 95, 75, 50, 25, 10 at
    both subsamplings, and stays between 15 and 60 dB; the Laplacian variance of the crop before and after quality 25 is printed."""
    qualities = (95.0, 75.0, 50.0, 25.0, 10.0)
    x = real_tile().unsqueeze(0).expand(len(qualities), -1, -1, -1).contiguous().to(dev)
    for sub in SUBS:
        out = jpeg_compress(x, qs(qualities, dev), subsampling=sub)
        mse = ((out.double() - x.double()) ** 2).mean(dim=(1, 2, 3)).cpu()
        psnr = (10.0 * torch.log10(255.0**2 / mse)).tolist()
        print(f"subsampling {sub}: PSNR over quality {qualities}: {[f'{v:.2f}' for v in psnr]} dB")
        assert all(a > b for a, b in zip(psnr, psnr[1:])), psnr
        assert 15.0 < psnr[-1] and psnr[0] < 60.0, psnr
        before, after = (focus_statistics(t).laplacian_variance().reshape(-1).cpu().tolist()[0] for t in (x[:1], out[3:4]))
        print(f"subsampling {sub}: Laplacian variance of the crop {before:.1f}, after quality 25 {after:.1f}")
        assert after > 0.0


# ------------------------------------------------------------------ the C ABI's refusals leave the output alone
def test_argument_errors_launch_nothing(dev, lib):
    x = tiles_u8((33, 31))[:3].contiguous().to(dev)
    out = torch.full_like(x, 7)
    quality, mask = qs((10.0, 50.0, 95.0), dev), torch.ones(3, 33, 31, dtype=torch.uint8, device=dev)
    code, stream, bad = _native.DTYPE_CODES[torch.uint8], _native.stream_ptr(dev), _native.SX_ERR_BAD_ARG
    p = lambda t: t.data_ptr()      # noqa: E731
    assert lib.sx_jpeg_roundtrip(None, p(out), code, 3, 33, 31, p(quality), 3, 2, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), None, code, 3, 33, 31, p(quality), 3, 2, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), p(out), code, 3, 33, 31, None, 3, 2, 0, stream) == bad and "null" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), p(out), code, 3, -33, 31, p(quality), 3, 2, 0, stream) == bad and "positive" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), p(out), code, 3, 33, 31, p(quality), 2, 2, 0, stream) == bad and "n_rows" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), p(out), code, 3, 33, 31, p(quality), 3, 1, 0, stream) == bad and "subsampling" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip_masked(p(x), p(out), code, 3, 33, 31, p(quality), 3, 2, None, 0, stream) == bad and "mask pointer is null" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip_masked(p(x), p(out), code, 3, 33, 31, p(quality), 3, 2, p(mask), CL, stream) == bad and "planar" in _native.last_error(lib)
    assert lib.sx_jpeg_roundtrip(p(x), p(out), 17, 3, 33, 31, p(quality), 3, 2, 0, stream) == _native.SX_ERR_DTYPE
    torch.cuda.synchronize(dev)
    assert bool((out == 7).all())
