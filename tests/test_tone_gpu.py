"""Tone augmentation on the GPU, through the C ABI (sx_tone_apply, sx_tone_apply_masked, sx_grey_statistics) and through ``adjust_tone`` /
``ToneAugment`` / ``grey_statistics``.

The yardstick is tests/_tone_numpy.py: the pixel rule and the generator in float64 on the float32 values the kernel reads, evaluated ONCE
per (element type, tile size, noise mode) and shared.  The bands are DESIGN.md 4v's, derived from the operation count and the stated
accuracy of log2f / exp2f / logf / sincospif (one unit in the last place each) and of the correctly rounded sqrtf -- not from what the
kernel gives:
  e = E_SMOOTH = 1e-3 levels   everywhere but below (the derivation gives 4e-4);
  e = E_ROOT   = 0.04 levels   float tiles under a row with gamma < 1 and b < 0: a x and 255 b cancel, the float32 level x = 255 v carries
                               an absolute error of up to 2^-24 x, and a power below 1 turns an absolute error d next to 0 into
                               sqrt(255 d) (0.034 at b = -0.3).  A uint8 tile's level is exact and 255 b is carried as a pair, so the
                               error of t is relative there and E_SMOOTH holds.
  uint8 output                 |out - level64| <= 0.5 + e for EVERY element;
  float32 / float64 tiles      e / 255 on [0, 1];  float16 / bfloat16: plus 2^-12 / 2^-9 (the HSV test's rounding term).  That term is half a unit
                               of the type at 1 on [0, 1]; a float tile's result is a LEVEL, and half a unit at 128..255 levels is 2^-4 / 0.5
                               levels, which is 255 / 256 of it more: e of a 16-bit tile carries the gap, 2.4e-4 / 1.95e-3 levels (SCALE_GAP);
  uint8 tiles, float outputs   the level is quantised to 8 bits first (the output rule): the uint8 band on 255 x out, widened by the half unit
                               of the output type where the / 255 is rounded to it.
A wrong Philox word, counter or channel assignment misses these bands by whole levels (255 sigma |z| is 2.5 to 25 levels at the sigmas
used): that is how the generator is pinned on the device.  Everything else is bit for bit.

Measured on an MI355X (the figures this file prints; README and DESIGN.md 4v quote them): uint8 output 0.50001 levels, float32 / float64 tiles
3.2e-7 on [0, 1] (8.3e-5 levels), float16 2.452e-4 and bfloat16 1.961e-3 (the rounding of a level to the type), uint8 tiles with ``/ 255`` to bf16
0.99313 and to f16 0.56132 levels; the mean pivot moved the grey mean by 0.044 levels."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import GaussianNoiseAugment, ToneAugment, _native, adjust_tone, grey_map, grey_statistics, level_histogram, tissue_mask
from tests import _hsv_numpy as hn
from tests import _tone_numpy as tn
from tests.test_hsv_gpu import graph_nodes, off_by_one

pytestmark = pytest.mark.gpu

E_SMOOTH, E_ROOT = 1e-3, 0.04
assert max(E_SMOOTH, E_ROOT) < 0.05      # (the condition on the derived band)
HALF_ULP_AT_1 = {torch.bfloat16: 2.0**-9, torch.float16: 2.0**-12, torch.float32: 0.0, torch.float64: 0.0}
SHAPES = ((1, 1), (1, 7), (2, 2), (5, 3), (33, 31), (64, 64), (65, 130))
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64)
DTYPE_IDS = [str(d).split(".")[-1] for d in DTYPES]
CL, UNIT = _native.MACENKO_CHANNELS_LAST, _native.MACENKO_NORMALIZE_0_1
OUT_FLAG = {torch.bfloat16: _native.MACENKO_OUT_BF16, torch.float16: _native.MACENKO_OUT_F16}
# (a, b, gamma, sigma): a in [0.5, 2], b in [-0.3, 0.3], gamma in {0.5, 1, 2}, sigma in {0, 0.02, 0.1}; two batches of three tiles
ROW_SETS = (((0.5, 0.3, 0.5, 0.02), (2.0, -0.3, 2.0, 0.1), (1.25, 0.1, 1.0, 0.0)),
            ((1.5, -0.2, 0.5, 0.1), (0.75, -0.05, 1.0, 0.02), (1.0, 0.0, 2.0, 0.0)))
SEED_SETS = ((1, -7, (1 << 62) + 12345), (0x123456789ABCDEF, 3 << 32, 99))
NAN_ROW = (float("nan"),) * 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ tiles and their references
@lru_cache(maxsize=None)
def tiles_of(dtype: torch.dtype, shape: tuple) -> torch.Tensor:
    """(3, 3, H, W) on the CPU.  uint8: seeded bytes; floats: seeded values in [0, 1] of the type (float64: float32 values), with a few
    below 0 and above 1 and -- from 5 x 3 up -- a NaN, an infinity and a pixel that is NaN in all channels."""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    if dtype == torch.uint8:
        return torch.from_numpy(rng.integers(0, 256, size=(3, 3, h, w), dtype=np.uint8))
    v = rng.random((3, 3, h, w), dtype=np.float32)
    flat = v.reshape(-1)
    if flat.size >= 45:
        flat[rng.integers(0, flat.size, size=max(flat.size // 50, 2))] = rng.uniform(-0.5, 1.5, size=max(flat.size // 50, 2)).astype(np.float32)
        v[0, 1, h // 2, w // 2], v[1, 2, 0, 1], v[2, :, h - 1, 0] = np.nan, np.inf, np.nan
    half = dtype if dtype in (torch.bfloat16, torch.float16) else torch.float32
    return torch.from_numpy(v).to(half).to(dtype)


# half a unit in the last place of a 16-bit level in [128, 256), in levels, less what the [0, 1] term of the band covers of it
SCALE_GAP = {torch.float16: 2.0**-4 - 255.0 * 2.0**-12, torch.bfloat16: 0.5 - 255.0 * 2.0**-9}
assert E_ROOT + max(SCALE_GAP.values()) < 0.05


def row_e(dtype: torch.dtype, row) -> float:
    return (E_ROOT if dtype != torch.uint8 and row[2] < 1.0 and row[1] < 0.0 else E_SMOOTH) + SCALE_GAP.get(dtype, 0.0)


@lru_cache(maxsize=None)
def reference(dtype: torch.dtype, shape: tuple, which: int, shared: bool) -> tuple[np.ndarray, np.ndarray]:
    """``(level64 (3, H*W, 3), copied (3, H*W))`` of the three tiles under row set ``which`` with its seeds."""
    x = tiles_of(dtype, shape)
    pixels = np.arange(shape[0] * shape[1])
    parts = [tn.levels64(hn.input_levels(x[t].permute(1, 2, 0).reshape(-1, 3)), ROW_SETS[which][t], SEED_SETS[which][t], pixels, shared) for t in range(3)]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def as_pixels(out: torch.Tensor, channels_last: bool) -> torch.Tensor:
    return (out if channels_last else out.permute(0, 2, 3, 1)).reshape(out.shape[0], -1, 3).cpu()


def layout(x: torch.Tensor, channels_last: bool, dev) -> torch.Tensor:
    return (x.permute(0, 2, 3, 1) if channels_last else x).contiguous().to(dev)


# ------------------------------------------------------------------ the raw calls
def out_dtype_of(x: torch.Tensor, flags: int) -> torch.dtype:
    if x.dtype == torch.uint8:
        for dtype, flag in OUT_FLAG.items():
            if flags & flag:
                return dtype
        return torch.float32 if flags & UNIT else torch.uint8
    return x.dtype


def raw(lib, x: torch.Tensor, rows: torch.Tensor, seeds: torch.Tensor | None = None, shared: bool = False, flags: int = 0, mask: torch.Tensor | None = None,
        out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_tone_apply / sx_tone_apply_masked on the current stream; ``rows``: (R, 4) float32, ``seeds``: (N,) int64 or None, on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype_of(x, flags), device=x.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == 4
    assert seeds is None or (seeds.dtype == torch.int64 and seeds.is_contiguous() and tuple(seeds.shape) == (n,))
    stream, code, s = _native.stream_ptr(x.device), _native.DTYPE_CODES[x.dtype], None if seeds is None else seeds.data_ptr()
    if mask is None:
        rc = lib.sx_tone_apply(x.data_ptr(), out.data_ptr(), code, n, h, w, rows.data_ptr(), rows.shape[0], s, int(shared), flags, stream)
    else:
        rc = lib.sx_tone_apply_masked(x.data_ptr(), out.data_ptr(), code, n, h, w, rows.data_ptr(), rows.shape[0], s, int(shared), mask.data_ptr(), flags, stream)
    assert rc == 0, _native.last_error(lib)
    return out


def raw_hsv(lib, x: torch.Tensor, flags: int = 0) -> torch.Tensor:
    """sx_hsv_apply under a NaN row: the copy."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    out = torch.empty(x.shape, dtype=out_dtype_of(x, flags), device=x.device)
    rows = torch.full((1, 5), float("nan"), dtype=torch.float32, device=x.device)
    rc = lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, rows.data_ptr(), 1, flags, _native.stream_ptr(x.device))
    assert rc == 0, _native.last_error(lib)
    return out


def row_tensor(rows, dev) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 4)


def seed_tensor(seeds, dev) -> torch.Tensor:
    return torch.tensor(seeds, dtype=torch.int64, device=dev)


# ------------------------------------------------------------------ against the float64 restatement
def check_levels(out: torch.Tensor, in_dtype: torch.dtype, unit: bool, level: np.ndarray, copied: np.ndarray, e: float, what) -> float:
    """``out``: (P, 3) on the CPU; ``level`` / ``copied``: the reference at the same pixels.  Prints the figure, then asserts."""
    got = out.to(torch.float64).numpy()
    assert np.isfinite(got).all(), what
    if in_dtype == torch.uint8:
        scale = 255.0 if unit else 1.0
        extra = 0.0 if out.dtype == torch.uint8 or not unit else 255.0 * HALF_ULP_AT_1[out.dtype]
        err = float(np.abs(got * scale - level).max())
        print(f"{what}: max |out - level64| = {err:.5f} levels (band {0.5 + e + extra:.4f})")
        assert err <= 0.5 + e + extra, (what, err)
        if out.dtype == torch.float32 or (out.dtype != torch.uint8 and not unit):      # the output rule: an 8-bit level, cast (divided by 255 in float32)
            q = torch.round(out.to(torch.float32) * scale)
            assert torch.equal(out, ((q / 255.0) if unit else q).to(out.dtype)), what
        return err
    assert not unit
    err = float(np.abs(got - level).max()) / 255.0
    bound = e / 255.0 + HALF_ULP_AT_1[out.dtype]
    print(f"{what}: max |out - level64| = {err:.3e} on [0, 1] (bound {bound:.3e})")
    assert err <= bound, (what, err)
    if copied.any():      # a pixel with a NaN member: the background rule's bits
        assert torch.equal(out[torch.from_numpy(copied)], hn.to_output(level[copied], in_dtype, out.dtype, False)), what
    return err


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_and_noise_against_float64(dev, lib, dtype, shape):
    """Three tiles, a row and a seed each, ONE launch: both noise modes, both layouts, both row sets."""
    for which in range(2):
        rows, seeds = row_tensor(ROW_SETS[which], dev), seed_tensor(SEED_SETS[which], dev)
        for shared in (False, True):
            level, copied = reference(dtype, shape, which, shared)
            for channels_last in (False, True):
                out = raw(lib, layout(tiles_of(dtype, shape), channels_last, dev), rows, seeds, shared, CL if channels_last else 0)
                assert out.dtype == dtype
                got = as_pixels(out, channels_last)
                for t in range(3):
                    check_levels(got[t], dtype, False, level[t], copied[t], row_e(dtype, ROW_SETS[which][t]), (DTYPE_IDS[DTYPES.index(dtype)], shape, which, shared, channels_last, t))
    if dtype != torch.uint8 and shape[0] * shape[1] >= 15:
        assert reference(dtype, shape, 0, False)[1].sum() >= 2      # (NaN members were among the pixels)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("flags", [OUT_FLAG[torch.bfloat16], OUT_FLAG[torch.float16], UNIT, UNIT | OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16]],
                         ids=["bf16", "f16", "unit_f32", "unit_bf16", "unit_f16"])
def test_uint8_tiles_float_outputs(dev, lib, flags, shape):
    rows, seeds = row_tensor(ROW_SETS[0], dev), seed_tensor(SEED_SETS[0], dev)
    for shared, channels_last in ((False, False), (True, True)):
        level, copied = reference(torch.uint8, shape, 0, shared)
        x = layout(tiles_of(torch.uint8, shape), channels_last, dev)
        out = raw(lib, x, rows, seeds, shared, flags | (CL if channels_last else 0))
        assert out.dtype == out_dtype_of(x, flags)
        got = as_pixels(out, channels_last)
        for t in range(3):
            check_levels(got[t], torch.uint8, bool(flags & UNIT), level[t], copied[t], E_SMOOTH, (flags, shape, shared, channels_last, t))
        if flags & UNIT and flags != UNIT:      # (the 16-bit / 255: the float32 quotient rounded to the type)
            assert torch.equal(out, raw(lib, x, rows, seeds, shared, UNIT | (CL if channels_last else 0)).to(out.dtype))


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
def test_normalize_0_1_divides_the_level_output_by_255(dev, lib, dtype):
    rows, seeds = row_tensor(ROW_SETS[1], dev), seed_tensor(SEED_SETS[1], dev)
    for shape in ((33, 31), (64, 64)):
        x = layout(tiles_of(dtype, shape), False, dev)
        level, unit = raw(lib, x, rows, seeds).cpu(), raw(lib, x, rows, seeds, flags=UNIT).cpu()      # (divided on the CPU: the IEEE quotient)
        want = level / 255.0 if dtype == torch.float64 else (level.to(torch.float32) / 255.0).to(dtype)
        assert torch.equal(unit, want), (dtype, shape)


# ------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_identity_copies_and_noise_free_forms(dev, lib, dtype, shape):
    x = layout(tiles_of(dtype, shape), False, dev)
    seeds = seed_tensor(SEED_SETS[0], dev)
    identity, nan_row = row_tensor(tn.IDENTITY, dev), row_tensor(NAN_ROW, dev)
    copy = raw(lib, x, nan_row)
    assert torch.equal(copy, raw_hsv(lib, x))      # the background rule's bits
    if dtype == torch.uint8:
        assert torch.equal(copy, x)
    for flags in ((0, UNIT) if dtype != torch.uint8 else (0, UNIT, OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16])):
        want = raw_hsv(lib, x, flags)
        assert torch.equal(raw(lib, x, identity, flags=flags), want), flags      # the identity row returns what a NaN row returns
        assert torch.equal(raw(lib, x, identity, seeds, flags=flags), want), flags      # sigma == 0 with seeds adds nothing
        for bad in ((float("nan"), 0.0, 1.0, 0.1), (1.2, float("inf"), 1.0, 0.1), (1.2, 0.1, float("-inf"), 0.1), (1.2, 0.1, 0.5, float("inf")), (1.2, 0.1, 0.0, 0.1),
                    (1.2, 0.1, -2.0, 0.1), (1.2, 0.1, 0.5, -0.01), (1.2, 0.1, 2.0, float("nan"))):
            for s in (None, seeds):
                assert torch.equal(raw(lib, x, row_tensor(bad, dev), s, flags=flags), want), (bad, flags)
    # a spoiled row leaves its tile and no other
    rows = row_tensor(ROW_SETS[0], dev)
    out = raw(lib, x, rows, seeds)
    for t in range(3):
        spoiled = rows.clone()
        spoiled[t, 2] = 0.0
        got = raw(lib, x, spoiled, seeds)
        others = [k for k in range(3) if k != t]
        assert torch.equal(got[t], copy[t]) and torch.equal(got[others], out[others]), t
    # seeds=None, sigma == 0 with seeds, and the kernel without the generator agree
    quiet = rows.clone()
    quiet[:, 3] = 0.0
    assert torch.equal(raw(lib, x, rows), raw(lib, x, quiet, seeds)) and torch.equal(raw(lib, x, rows), raw(lib, x, quiet))
    # the same seed twice agrees; another seed differs (where there is noise to differ: more than a few pixels)
    assert torch.equal(raw(lib, x, rows, seeds), out)
    if shape[0] * shape[1] >= 15:
        other = raw(lib, x, rows, seeds + 1)
        assert not torch.equal(other[0], out[0]) and not torch.equal(other[1], out[1]) and torch.equal(other[2], out[2])      # (tile 2: sigma == 0)
        assert not torch.equal(raw(lib, x, rows, seeds, True), out)
    # a tile alone is that tile in the batch, with its row and seed; one row for the batch is that row for every tile
    for shared in (False, True):
        batch = raw(lib, x, rows, seeds, shared)
        for t in range(3):
            assert torch.equal(batch[t:t + 1], raw(lib, x[t:t + 1].contiguous(), rows[t:t + 1].contiguous(), seeds[t:t + 1].contiguous(), shared)), (shared, t)
    assert torch.equal(raw(lib, x, rows[1:2].contiguous(), seeds), raw(lib, x, rows[1:2].repeat(3, 1), seeds))
    # NCHW and NHWC give the same values
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(raw(lib, nhwc, rows, seeds, flags=CL).permute(0, 3, 1, 2), out)
    # a view one element off (the scalar path) equals the aligned call
    assert torch.equal(raw(lib, off_by_one(x), rows, seeds), out)
    assert torch.equal(raw(lib, x, rows, seeds, out=off_by_one(torch.empty_like(out))), out)
    assert torch.equal(raw(lib, off_by_one(nhwc), rows, seeds, flags=CL).permute(0, 3, 1, 2), out)
    # shared noise on a tile with r = g = b gives three equal planes
    grey = x[:, :1].expand(-1, 3, -1, -1).contiguous()
    same = raw(lib, grey, rows, seeds, True)
    assert torch.equal(same[:, 0], same[:, 1]) and torch.equal(same[:, 0], same[:, 2])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_masks(dev, lib, dtype, shape):
    x = layout(tiles_of(dtype, shape), False, dev)
    rows, seeds = row_tensor(ROW_SETS[1], dev), seed_tensor(SEED_SETS[1], dev)
    plain, copy = raw(lib, x, rows, seeds), raw(lib, x, row_tensor(NAN_ROW, dev))
    assert torch.equal(raw(lib, x, rows, seeds, mask=torch.ones(3, *shape, dtype=torch.uint8, device=dev)), plain)
    assert torch.equal(raw(lib, x, rows, seeds, mask=torch.zeros(3, *shape, dtype=torch.uint8, device=dev)), copy)
    mask = (torch.rand(3, *shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.6).to(torch.uint8) * 255      # (non-zero = in)
    got = raw(lib, x, rows, seeds, mask=mask)
    inside = mask.bool().unsqueeze(1)
    assert torch.equal(got, torch.where(inside, plain, copy))      # masked-out: the copy; masked-in: the unmasked call's bits (the noise does not see the mask)
    assert torch.equal(raw(lib, x, rows, seeds, mask=off_by_one(mask)), got) and torch.equal(raw(lib, off_by_one(x), rows, seeds, mask=mask), got)
    # values under masked-out pixels do not matter
    junk = x.clone()
    out_px = ~inside.expand_as(x)
    junk[out_px] = torch.tensor(float("nan") if dtype != torch.uint8 else 7).to(dtype)
    assert torch.equal(raw(lib, junk, rows, seeds, mask=mask)[~out_px], got[~out_px])
    for flags in ((UNIT,) if dtype != torch.uint8 else (UNIT, OUT_FLAG[torch.bfloat16])):
        assert torch.equal(raw(lib, x, rows, seeds, True, flags, mask=mask), torch.where(inside, raw(lib, x, rows, seeds, True, flags), raw_hsv(lib, x, flags)))


# ------------------------------------------------------------------ grey statistics
def sums_of_histogram(counts: torch.Tensor) -> torch.Tensor:
    """(rows, 256) int64 counts -> (rows, 3) int64 [pixels, sum Y, sum Y^2]."""
    levels = torch.arange(256, dtype=torch.int64, device=counts.device)
    return torch.stack([counts.sum(dim=1), (counts * levels).sum(dim=1), (counts * levels * levels).sum(dim=1)], dim=1)


def words_of(stats) -> torch.Tensor:
    return torch.stack([stats.pixels, stats.sum, stats.sum_squares], dim=1)


@pytest.mark.parametrize("shape", ((1, 1), (5, 3), (33, 31), (64, 64), (65, 130)), ids=["1x1", "5x3", "33x31", "64x64", "65x130"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_grey_statistics(dev, dtype, shape):
    x = layout(tiles_of(dtype, shape), False, dev)      # (float tiles from 5 x 3 up hold NaN pixels: Y = 0, counted)
    grey = grey_map(x)
    for pooled in (False, True):
        want = sums_of_histogram(level_histogram(grey, pooled=pooled).counts)
        got = grey_statistics(x, pooled=pooled)
        assert all(word.dtype == torch.int64 and tuple(word.shape) == ((1,) if pooled else (3,)) for word in got)
        assert torch.equal(words_of(got), want), (pooled, words_of(got), want)
        assert int(got.pixels.sum()) == 3 * shape[0] * shape[1]
        assert torch.equal(words_of(grey_statistics(x.permute(0, 2, 3, 1).contiguous(), pooled=pooled, channel_axis=-1)), want)
        assert torch.equal(words_of(grey_statistics(off_by_one(x), pooled=pooled)), want)
    # under a mask: the histogram of the masked-in levels, in torch; tile 1 is masked out altogether
    mask = (torch.rand(3, *shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) < 0.5).to(torch.uint8) * 3
    mask[1] = 0
    per_tile = torch.stack([torch.bincount(grey[t][mask[t] != 0].to(torch.int64), minlength=256) for t in range(3)])
    got = grey_statistics(x, mask=mask)
    assert torch.equal(words_of(got), sums_of_histogram(per_tile)) and got.pixels[1].item() == 0
    assert torch.equal(words_of(grey_statistics(x, mask=mask.bool().unsqueeze(1), pooled=True)), sums_of_histogram(per_tile.sum(dim=0, keepdim=True)))
    assert torch.equal(words_of(grey_statistics(x, mask=off_by_one(mask))), sums_of_histogram(per_tile))
    assert torch.isnan(got.mean()[1]) and torch.isnan(got.rms_contrast()[1])
    if dtype == torch.uint8:
        rule, _ = tissue_mask(x, 0.7)
        assert torch.equal(words_of(grey_statistics(x, mask="luminosity", luminosity_threshold=0.7)), words_of(grey_statistics(x, mask=rule)))
        whole = grey_statistics(x)
        values = grey.to(torch.float64).reshape(3, -1)
        assert torch.allclose(whole.mean(), values.mean(dim=1), rtol=0, atol=1e-9) and torch.allclose(whole.rms_contrast(), values.std(dim=1, unbiased=False), rtol=0, atol=1e-7)


def test_a_captured_grey_statistics_replays_on_new_images(dev):
    first, second = layout(tiles_of(torch.uint8, (65, 130)), False, dev), layout(tiles_of(torch.uint8, (65, 130)).flip(0).contiguous() // 2, False, dev)
    want_first, want_second = words_of(grey_statistics(first)), words_of(grey_statistics(second))
    assert not torch.equal(want_first, want_second)
    buf = first.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        grey_statistics(buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = words_of(grey_statistics(buf))
        types = graph_nodes(dev)[0]
    assert 2 not in types, types      # no memset node (hipGraphNodeTypeMemset = 2): the words are cleared by a launch while capturing
    for images, want in ((first, want_first), (second, want_second), (first, want_first)):
        buf.copy_(images)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want)


# ------------------------------------------------------------------ the modules
def test_module_and_functional_form(dev, lib):
    x = layout(tiles_of(torch.uint8, (33, 31)), False, dev)
    rows, seeds = row_tensor(ROW_SETS[0], dev), seed_tensor(SEED_SETS[0], dev)
    want = raw(lib, x, rows, seeds)
    assert torch.equal(adjust_tone(x, rows, seeds=seeds), want) and torch.equal(adjust_tone(x, rows), raw(lib, x, rows))
    assert torch.equal(adjust_tone(x, rows, seeds=seeds, shared_noise=True), raw(lib, x, rows, seeds, True))
    with pytest.raises(ValueError, match="runs on a CUDA"):
        adjust_tone(x.cpu(), rows)
    aug = ToneAugment(normalize_to_0_1=False)
    assert torch.equal(aug(x, rows, seeds), want)
    assert torch.equal(ToneAugment()(x, rows, seeds), raw(lib, x, rows, seeds, flags=UNIT))      # normalize_to_0_1 defaults to True, as HSVAugment's
    assert torch.equal(adjust_tone(x, rows, seeds=seeds, out_dtype=torch.bfloat16), raw(lib, x, rows, seeds, flags=OUT_FLAG[torch.bfloat16]))
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(adjust_tone(nhwc, rows, seeds=seeds, channel_axis=-1), want.permute(0, 2, 3, 1))
    one = raw(lib, x, rows[1:2].contiguous(), seeds)
    assert torch.equal(adjust_tone(x, rows[1], seeds=seeds), one) and torch.equal(adjust_tone(x, rows[1:2], seeds=seeds), one) and torch.equal(aug(x, rows[1].cpu(), seeds.cpu()), one)
    single = aug(x[1], rows[1], seeds[1:2])      # CHW in, CHW out
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, want[1])
    # masks: the rule is the explicit tissue mask
    explicit, counts = tissue_mask(x, 0.7)
    assert 0 < int(counts.sum()) < explicit.numel()
    masked = adjust_tone(x, rows, seeds=seeds, mask=explicit)
    assert torch.equal(adjust_tone(x, rows, seeds=seeds, mask="luminosity", luminosity_threshold=0.7), masked)
    assert torch.equal(ToneAugment(mask="luminosity", luminosity_threshold=0.7, normalize_to_0_1=False)(x, rows, seeds), masked)
    assert torch.equal(aug(x, rows, seeds, mask=explicit.unsqueeze(1)), masked) and not torch.equal(masked, want)
    # p = 0 is the copy; zero magnitudes are the identity rows
    assert torch.equal(ToneAugment(p=0.0, noise=0.1, normalize_to_0_1=False)(x), x)
    assert torch.equal(ToneAugment(0.0, 0.0, normalize_to_0_1=False)(x), x) and torch.equal(GaussianNoiseAugment(0.0, normalize_to_0_1=False)(x), x)
    # a draw: forward is adjust_tone with sample_rows / sample_seeds from an equal generator, on the device when the generator is there
    for where in ("cpu", dev):
        for kwargs in ({"pivot": "mean"}, {"pivot": 0.5, "shared_noise": True}, {"pivot": "mean", "mask": "luminosity", "luminosity_threshold": 0.7}):
            make = lambda: ToneAugment(0.2, 0.3, shift=0.05, gamma=0.3, noise=0.05, p=0.6, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5), **kwargs)      # noqa: E731
            got, again = make()(x), make()
            means = None
            if kwargs["pivot"] == "mean":
                means = grey_statistics(x, mask=kwargs.get("mask"), luminosity_threshold=0.7).mean()
            rows_again = again.sample_rows(3, means, dev)
            seeds_again = again.sample_seeds(3, dev)
            assert torch.equal(got, adjust_tone(x, rows_again, seeds=seeds_again, shared_noise=kwargs.get("shared_noise", False), mask=kwargs.get("mask"), luminosity_threshold=0.7))
            left = torch.isnan(rows_again).any(dim=1)
            assert torch.equal(got[left], x[left])
        noise = lambda: GaussianNoiseAugment((0.01, 0.05), normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(9))      # noqa: E731
        again = noise()
        assert torch.equal(noise()(x), adjust_tone(x, again.sample_rows(3, None, dev), seeds=again.sample_seeds(3, dev)))
    # a tile with no counted pixel gets a NaN row and is copied
    none_in = torch.ones(3, 33, 31, dtype=torch.uint8, device=dev)
    none_in[2] = 0
    out = ToneAugment(0.3, 0.3, normalize_to_0_1=False)(x, mask=none_in)
    assert torch.equal(out[2], x[2]) and not torch.equal(out[0], x[0])


def test_mean_pivot_keeps_the_grey_mean(dev):
    """Contrast alone about the tile's own mean on mid-grey tiles that no clamp touches: the grey mean stays within one level."""
    gen = torch.Generator().manual_seed(21)
    x = torch.randint(96, 161, (8, 3, 64, 64), generator=gen, dtype=torch.uint8).to(dev)
    aug = ToneAugment(0.0, 0.4, normalize_to_0_1=False, generator=torch.Generator().manual_seed(4))
    out = aug(x)
    before, after = grey_statistics(x), grey_statistics(out)
    assert int(out.min()) > 0 and int(out.max()) < 255 and not torch.equal(out, x)
    drift = float((after.mean() - before.mean()).abs().max())
    spread = (after.rms_contrast() / before.rms_contrast()).cpu()
    print(f"mean pivot: max |grey mean after - before| = {drift:.4f} levels; contrast ratios {spread.min():.3f} .. {spread.max():.3f}")
    assert drift <= 1.0 and float(spread.max() - spread.min()) > 0.2      # (and the contrast did change, tile by tile)


def test_a_captured_forward_replays_with_new_rows_seeds_and_images(dev):
    first, second = layout(tiles_of(torch.uint8, (64, 64)), False, dev), layout(tiles_of(torch.uint8, (64, 64)).flip(0).contiguous(), False, dev)
    rows_a, rows_b = row_tensor(ROW_SETS[0], dev), row_tensor(ROW_SETS[1], dev)
    seeds_a, seeds_b = seed_tensor(SEED_SETS[0], dev), seed_tensor(SEED_SETS[1], dev)
    for mode, nodes in ((None, [0]), ("luminosity", [0, 0])):      # ONE kernel node (hipGraphNodeTypeKernel = 0); two under the luminosity rule (the mask launch)
        aug = ToneAugment(noise=0.1, normalize_to_0_1=False, mask=mode, luminosity_threshold=0.7)
        want_a, want_b = aug(first, rows_a, seeds_a), aug(second, rows_b, seeds_b)
        assert not torch.equal(want_a, want_b)
        x, rows, seeds = first.clone(), rows_a.clone(), seeds_a.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):      # (warm-up on the capture stream)
            aug(x, rows, seeds)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = aug(x, rows, seeds)
            types, roots, edges = graph_nodes(dev)
        assert types == nodes, types      # no memset node (2), no copy (1)
        assert roots == 1 and edges == len(nodes) - 1      # a single branch
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want_a)
        x.copy_(second), rows.copy_(rows_b), seeds.copy_(seeds_b)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want_b)
