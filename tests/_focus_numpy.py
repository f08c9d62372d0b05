"""Numpy restatements for focus measurement (tests/test_focus_cpu.py pins them to scipy and to exact rationals, tests/test_focus_gpu.py
compares the device with them, exactly): the grey level in int64 from the levels of tests/_saturation_numpy.py, the Laplacian and the
Sobel responses on an ``np.pad(mode="reflect")`` of the grey map, the four sums per cell, and a cell grid as a pixel mask by ``np.repeat``
and a crop.  Also the inputs both test files share."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import _masked_numpy as mn
from tests._saturation_numpy import as_numpy, levels_of      # noqa: F401  (as_numpy: re-exported for the GPU tests)

BLOCK = (64, 64)                      # the statistics kernel's block (csrc/focus.hpp: kFocusRows x kFocusCols); a wave takes a band of 16 rows
MAIN_SHAPE = (3, 150, 203)            # two full blocks and a ragged remainder both ways (150 = 2 * 64 + 22, 203 = 3 * 64 + 11); 203 % 4 != 0
SMALL_SHAPES = ((1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 2, 2), (2, 5, 4))      # axes of length 1 and 2, where the reflection can go wrong
ALIGNED_SHAPES = ((2,) + BLOCK, (2, BLOCK[0], 2 * BLOCK[1]), (1, 2 * BLOCK[0], BLOCK[1]))      # exactly one block, exactly two (either way): the 4-wide loads
BLOCKS = (None, (8, 8), (16, 32), (64, 64), (128, 64), (64, 192))
MAX_L = 1020
MAX_T = 2 * 1020 * 1020


# ------------------------------------------------------------------ the rules
def grey_of_levels(r: np.ndarray, g: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (4899 * r.astype(np.int64) + 9617 * g.astype(np.int64) + 1868 * b.astype(np.int64) + 8192) >> 14


def grey_map(images: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """(N, H, W) uint8 of (N, 3, H, W) (channel_axis=-1: (N, H, W, 3)) images of any element type numpy holds (bf16: pass float32, exact)."""
    lv, nan = levels_of(images)
    lv = np.moveaxis(lv, channel_axis, 0)
    y = grey_of_levels(lv[0], lv[1], lv[2])
    assert y.min(initial=0) >= 0 and y.max(initial=0) <= 255
    return np.where(nan.any(axis=channel_axis), 0, y).astype(np.uint8)


def stencils(grey: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(L, T) int64 of an (N, H, W) uint8 grey map: the 5-point Laplacian and Gx^2 + Gy^2 of the 3 x 3 Sobel responses, the border reflected
    without repeating the edge, every tile on its own."""
    assert grey.ndim == 3 and grey.dtype == np.uint8
    n, h, w = grey.shape
    p = np.pad(grey.astype(np.int64), ((0, 0), (1, 1), (1, 1)), mode="reflect")

    def at(dy: int, dx: int) -> np.ndarray:
        return p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    lap = at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1) - 4 * at(0, 0)
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return lap, gx * gx + gy * gy


def statistics_of_grey(grey: np.ndarray, block=None, mask: np.ndarray | None = None, pooled: bool = False) -> np.ndarray:
    """(4, N, gh, gw) int64 -- pixels, sum L, sum L^2, sum T per cell -- or (4, 1, 1, 1) pooled."""
    n, h, w = grey.shape
    lap, ten = stencils(grey)
    inside = np.ones((n, h, w), dtype=np.int64) if mask is None else (np.asarray(mask).reshape(n, h, w) != 0).astype(np.int64)
    bh, bw = (h, w) if block is None else block
    gh, gw = -(-h // bh), -(-w // bw)
    out = np.zeros((4, n, gh, gw), dtype=np.int64)
    for k, word in enumerate((inside, inside * lap, inside * lap * lap, inside * ten)):
        padded = np.zeros((n, gh * bh, gw * bw), dtype=np.int64)
        padded[:, :h, :w] = word
        out[k] = padded.reshape(n, gh, bh, gw, bw).sum(axis=(2, 4))
    return out.sum(axis=(1, 2, 3), keepdims=True) if pooled else out


def statistics(images: np.ndarray, block=None, mask: np.ndarray | None = None, pooled: bool = False, channel_axis: int = 1) -> np.ndarray:
    return statistics_of_grey(grey_map(images, channel_axis), block, mask, pooled)


def variance_exact(pixels: int, sums: int, squares: int):
    """The population variance as an exact rational (a Fraction), None for an empty cell."""
    from fractions import Fraction

    if pixels == 0:
        return None
    return Fraction(squares, pixels) - Fraction(sums, pixels) ** 2


def cells_mask(cells: np.ndarray, height: int, width: int, block, mask: np.ndarray | None = None) -> np.ndarray:
    big = np.repeat(np.repeat(cells != 0, block[0], axis=1), block[1], axis=2)[:, :height, :width]
    if mask is not None:
        big = big & (np.asarray(mask).reshape(big.shape) != 0)
    return big.astype(np.uint8)


def box_blur(images_u8: np.ndarray, size: int = 3) -> np.ndarray:
    """A size x size box blur of (N, 3, H, W) uint8 tiles, edges replicated, rounded half up: what defocus is stood in for here."""
    half = size // 2
    p = np.pad(images_u8.astype(np.int64), ((0, 0), (0, 0), (half, half), (half, half)), mode="edge")
    h, w = images_u8.shape[2:]
    total = sum(p[:, :, dy:dy + h, dx:dx + w] for dy in range(size) for dx in range(size))
    return ((2 * total + size * size) // (2 * size * size)).astype(np.uint8)


# ------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def real_crop(rows: int = 150, cols: int = 203, count: int = 3) -> np.ndarray:
    """(count, 3, rows, cols) uint8: the crop of the real fixture that tests/_saturation_numpy.real_saturation uses."""
    images, _ = mn.real_images()
    out = np.ascontiguousarray(images[:count, :, 300:300 + rows, 100:100 + cols].numpy())
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tiles_u8(shape: tuple[int, int, int] = MAIN_SHAPE) -> np.ndarray:
    """(N, 3, H, W) uint8 with DIFFERENT tiles: real tissue or noise first, then (N > 1) a constant tile, then (N > 2) a checkerboard of the
    levels 0 and 255 in all three channels, the extreme L and T; any further tiles are noise."""
    n, h, w = shape
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    out = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    if shape == MAIN_SHAPE:
        out[0] = real_crop()[0]
    if n > 1:
        out[1] = np.array([200, 100, 50], dtype=np.uint8)[:, None, None]
    if n > 2:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        out[2] = np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)[None]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tiles_mask(shape: tuple[int, int, int] = MAIN_SHAPE, kind: str = "random") -> np.ndarray:
    n, h, w = shape
    if kind == "ones":
        out = np.ones(shape, dtype=np.uint8)
    elif kind == "zeros":
        out = np.zeros(shape, dtype=np.uint8)
    else:      # bytes of any non-zero value count as set
        rng = np.random.default_rng(5)
        out = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, shape, dtype=np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(shape: tuple[int, int, int] = MAIN_SHAPE, block=None, mask_kind: str | None = None, pooled: bool = False) -> np.ndarray:
    """The restatement's statistics of tiles_u8(shape): computed once per case and shared."""
    out = statistics(tiles_u8(shape), block, None if mask_kind is None else tiles_mask(shape, mask_kind), pooled)
    out.setflags(write=False)
    return out


def as_torch(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(words))      # (a copy: the shared results are read-only)
