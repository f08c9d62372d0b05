"""Numpy restatements for saturation-channel tissue detection (tests/test_saturation_cpu.py pins them, tests/test_saturation_gpu.py compares
the device with them, exactly): the 8-bit level of a stored element, the saturation rule in int64, the median as a partition of a
sliding window over an edge-padded array, the histogram as a bincount and the mask as ``>``.  Also the inputs both test files share."""
from __future__ import annotations

import functools

import numpy as np
import torch

from stainx_amd import synth
from tests import _masked_numpy as mn

SIZES = (3, 5, 7, 9, 11, 13, 15)
BLOCK = (64, 64)                      # the median kernel's output block (csrc/saturation.hpp: kMedianRows x kMedianCols)
MAIN_SHAPE = (3, 150, 203)            # two full blocks and a ragged remainder both ways (150 = 2 * 64 + 22, 203 = 3 * 64 + 11); 203 % 4 != 0
SMALL_SHAPES = ((1, 1, 1), (2, 2, 5), (4, 1, 130), (4, 130, 1), (1,) + BLOCK)      # sizes 3 and 15 on each; the last is exactly one block
GENERATORS = ("random", "constant", "hramp", "vramp", "salt_pepper", "checkerboard", "mask01", "real")
MAP_SHAPES = ((3, 30, 30), (2, 33, 47), (1, 5, 4))


# ------------------------------------------------------------------ levels and saturation
def levels_of(images: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(levels int64, nan bool) of stored elements: a uint8 is its own level, anything else rint(clip(255 * float32(v), 0, 255)) in float32."""
    if images.dtype == np.uint8:
        return images.astype(np.int64), np.zeros(images.shape, dtype=bool)
    v = images.astype(np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        lv = np.rint(np.clip(np.float32(255) * np.where(nan, np.float32(0), v), np.float32(0), np.float32(255)))
    assert lv.dtype == np.float32
    return lv.astype(np.int64), nan


def saturation_of_levels(hi: np.ndarray, lo: np.ndarray) -> np.ndarray:
    hi, lo = hi.astype(np.int64), lo.astype(np.int64)
    return np.where(hi == 0, 0, (510 * (hi - lo) + hi) // np.maximum(2 * hi, 1))


def saturation_map(images: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """(N, H, W) uint8 of (N, 3, H, W) (channel_axis=-1: (N, H, W, 3)) images of any element type numpy holds (bf16: pass float32, exact)."""
    lv, nan = levels_of(images)
    s = saturation_of_levels(lv.max(axis=channel_axis), lv.min(axis=channel_axis))
    return np.where(nan.any(axis=channel_axis), 0, s).astype(np.uint8)


def as_numpy(x: torch.Tensor) -> np.ndarray:
    return x.numpy() if x.dtype in (torch.uint8, torch.float32, torch.float64, torch.float16) else x.float().numpy()      # (bf16 -> float32 is exact)


# ------------------------------------------------------------------ median, histogram, mask
def median(levels: np.ndarray, size: int) -> np.ndarray:
    """(N, H, W) uint8: the value of rank (size^2 + 1) / 2 of each size x size window, borders replicated, tiles independent."""
    assert levels.ndim == 3 and levels.dtype == np.uint8 and size % 2 == 1
    half = size // 2
    padded = np.pad(levels, ((0, 0), (half, half), (half, half)), mode="edge")
    out = np.empty_like(levels)
    for i in range(levels.shape[0]):      # (a tile at a time: the windows of one tile are size^2 times its bytes)
        windows = np.lib.stride_tricks.sliding_window_view(padded[i], (size, size)).reshape(levels.shape[1], levels.shape[2], size * size)
        rank = (size * size + 1) // 2
        out[i] = np.partition(windows, rank - 1, axis=-1)[..., rank - 1]
    return out


def majority(mask01: np.ndarray, size: int) -> np.ndarray:
    """The majority filter of a 0 / 1 map by window SUMS (an integral image, no sorting): 1 where the ones reach the rank."""
    half = size // 2
    padded = np.pad(mask01.astype(np.int64), ((0, 0), (half, half), (half, half)), mode="edge")
    integral = np.pad(padded.cumsum(axis=1).cumsum(axis=2), ((0, 0), (1, 0), (1, 0)))
    h, w = mask01.shape[1:]
    sums = integral[:, size:size + h, size:size + w] - integral[:, :h, size:size + w] - integral[:, size:size + h, :w] + integral[:, :h, :w]
    return (sums >= (size * size + 1) // 2).astype(np.uint8)


def histogram(levels: np.ndarray) -> np.ndarray:
    return np.stack([np.bincount(tile.reshape(-1), minlength=256) for tile in levels]).astype(np.int64)


def mask(levels: np.ndarray, thresholds) -> np.ndarray:
    return (levels.astype(np.int64) > np.asarray(thresholds, dtype=np.int64).reshape(-1, 1, 1)).astype(np.uint8)


# ------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def real_saturation(rows: int = 150, cols: int = 203, count: int = 3) -> np.ndarray:
    """A crop of the real fixture's saturation map, from inside the tissue of its first images."""
    images, _ = mn.real_images()
    return saturation_map(images[:count, :, 300:300 + rows, 100:100 + cols].numpy())


@functools.lru_cache(maxsize=None)
def levels_case(name: str, shape: tuple[int, int, int] = MAIN_SHAPE) -> np.ndarray:
    n, h, w = shape
    rng = np.random.default_rng(GENERATORS.index(name) + 31)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if name == "random":
        out = rng.integers(0, 256, shape)
    elif name == "constant":
        out = np.full(shape, 137)
    elif name == "hramp":
        out = np.broadcast_to(xx * 255 // max(w - 1, 1), shape)
    elif name == "vramp":
        out = np.broadcast_to(yy * 255 // max(h - 1, 1), shape)
    elif name == "salt_pepper":
        noise = rng.random(shape)
        out = np.where(noise < 0.025, 0, np.where(noise < 0.05, 255, 128))
    elif name == "checkerboard":
        out = np.broadcast_to(np.where((yy + xx) % 2 == 0, 50, 200), shape)      # two levels: ties at the rank
    elif name == "mask01":
        out = rng.random(shape) < 0.5
    elif name == "real":
        assert shape == MAIN_SHAPE
        out = real_saturation()
    else:
        raise KeyError(name)
    out = np.ascontiguousarray(out).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def median_case(name: str, size: int, shape: tuple[int, int, int] = MAIN_SHAPE) -> np.ndarray:
    out = median(levels_case(name, shape), size)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def map_tiles_u8(kind: str, index: int) -> torch.Tensor:
    """(N, 3, H, W) uint8 inputs of the saturation-map tests: synthetic H&E and random bytes on MAP_SHAPES."""
    n, h, w = MAP_SHAPES[index]
    return synth.he_batch(n, h, w, seed0=400 + index, scale_step=0.05) if kind == "he" else synth.noise_u8((n, 3, h, w), 143 + index)


def ladder_u8() -> torch.Tensor:
    """(1, 3, 3, 256) uint8: M = 0..255 along a row, with m = 0, m = M and m = max(M - 1, 0) in the three rows; the channels hold (M, m, mid)."""
    big = np.arange(256)
    rows = []
    for small in (np.zeros(256, dtype=np.int64), big, np.maximum(big - 1, 0)):
        rows.append(np.stack([big, small, (big + small) // 2]))
    tile = np.stack(rows, axis=1)[None]      # (1, 3, 3, 256)
    return torch.from_numpy(tile.astype(np.uint8))


def special_floats(dtype: torch.dtype) -> torch.Tensor:
    """(1, 3, 4, 6) float tile: values below 0 and above 1, +-inf, and a NaN in one channel of some pixels."""
    inf, nan = float("inf"), float("nan")
    values = [-0.5, 0.0, 0.25, 0.5, 1.0, 1.5, inf, -inf, nan, 0.1, 0.9, 2.0 / 255.0, 0.5 / 255.0, 1.5 / 255.0, 254.5 / 255.0, -0.0, 1e-30, 3.0]
    rng = np.random.default_rng(77)
    picks = rng.integers(0, len(values), (1, 3, 4, 6))
    tile = np.array(values, dtype=np.float64)[picks]
    tile[0, :, 0, 0] = (0.2, nan, 0.7)      # a NaN in one channel
    tile[0, :, 0, 1] = (inf, 0.0, 0.5)
    tile[0, :, 0, 2] = (-inf, 0.5, 1.0)
    tile[0, :, 0, 3] = (1.7, -0.3, 0.4)
    tile[0, :, 0, 4] = (inf, inf, -inf)
    tile[0, :, 0, 5] = (nan, nan, nan)
    return torch.from_numpy(tile).to(dtype)
