"""The yardsticks of the tissue-detection tests, restated without the library: Otsu's threshold with ``fractions.Fraction``, binary
morphology as numpy shifts over a padded array (tests/test_tissue_detect_cpu.py pins it to scipy.ndimage), and the oracle's luminosity
histogram -- bin ``floor(L / 255 * 256)`` of the CPU oracle's lightness -- with the count of pixels it cannot decide at each cut.  Also the
inputs both test files use."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np
import torch

from stainx_amd import synth
from tests import _masked_numpy as mn

L_BAND = mn.L_BAND      # oracle lightness nearer than this to a cut (0..255 scale): the oracle does not decide the pixel
BAND_CAP = 1e-2         # ... and at most this share of an input's pixels may lie that near to any ONE of the 255 cuts
MAX_RADIUS = 31
OPS = ("erode", "dilate", "open", "close")
ELEMENTS = ("square", "disk")


# ------------------------------------------------------------------ Otsu
def otsu_maximisers(counts) -> list[int]:
    """The k in 1..255 that reach the maximum of Otsu's between-class variance w0 w1 (mu0 - mu1)^2 for one row of 256 integer counts, in
    exact rational arithmetic: class 0 is the bins < k, the means are taken over the bin indices, and a k counts only with both classes
    populated."""
    counts = [int(c) for c in counts]
    total = sum(counts)
    best, ks = None, []
    for k in range(1, 256):
        n0, n1 = sum(counts[:k]), sum(counts[k:])
        if n0 == 0 or n1 == 0:
            continue
        mu0 = Fraction(sum(i * c for i, c in enumerate(counts[:k])), n0)
        mu1 = Fraction(sum(i * c for i, c in enumerate(counts[k:], start=k)), n1)
        var = Fraction(n0, total) * Fraction(n1, total) * (mu0 - mu1) ** 2
        if best is None or var > best:
            best, ks = var, [k]
        elif var == best:
            ks.append(k)
    return ks


def otsu_k(counts, fallback_k=None):
    """(k_first + k_last) // 2 of the maximisers; none: ``fallback_k``."""
    ks = otsu_maximisers(counts)
    return (ks[0] + ks[-1]) // 2 if ks else fallback_k


def otsu_thresholds(counts: np.ndarray, fallback: float = 0.8) -> np.ndarray:
    out = []
    for row in counts:
        k = otsu_k(row)
        out.append(fallback if k is None else k / 256.0)
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------ morphology
def half_widths(radius: int, element: str) -> list[int]:
    """half[|dy|]: the element's row at height dy is the offsets dx = -half..half."""
    if element == "square":
        return [radius] * (radius + 1)
    return [math.isqrt(radius * radius - a * a) for a in range(radius + 1)]


def footprint(radius: int, element: str) -> np.ndarray:
    """The element as a (2r+1, 2r+1) boolean array (scikit-image's ``disk(r)`` / ``square(2r+1)``)."""
    ax = np.arange(-radius, radius + 1)
    if element == "square":
        return np.ones((2 * radius + 1, 2 * radius + 1), dtype=bool)
    return (ax[:, None] ** 2 + ax[None, :] ** 2) <= radius * radius


def _sweep(mask: np.ndarray, radius: int, element: str, erode: bool) -> np.ndarray:
    """Erosion (AND over the element's offsets, outside = set) or dilation (OR, outside = unset) of (N, H, W) boolean masks: shifted views
    of the array padded by the radius -- first along a row, half-width by half-width, then the rows that take each half-width."""
    n, h, w = mask.shape
    r = radius
    padded = np.pad(mask, ((0, 0), (r, r), (r, r)), constant_values=erode)
    join = np.logical_and if erode else np.logical_or
    half = half_widths(r, element)
    out = np.full((n, h, w), erode, dtype=bool)
    along = padded[:, :, r:r + w].copy()      # (N, H + 2r, W): the row sweep of half-width 0
    for width in range(0, r + 1):
        if width:
            along = join(join(along, padded[:, :, r + width:r + width + w]), padded[:, :, r - width:r - width + w])
        for a in range(r + 1):
            if half[a] == width:
                for dy in {a, -a}:
                    out = join(out, along[:, r + dy:r + dy + h])
    return out


def morphology(mask: np.ndarray, op: str, radius: int, element: str) -> np.ndarray:
    """(N, H, W) boolean result of ``op`` on (N, H, W) masks (non-zero = set)."""
    m = np.asarray(mask) != 0
    if op == "erode":
        return _sweep(m, radius, element, True)
    if op == "dilate":
        return _sweep(m, radius, element, False)
    if op == "open":
        return _sweep(_sweep(m, radius, element, True), radius, element, False)
    if op == "close":
        return _sweep(_sweep(m, radius, element, False), radius, element, True)
    raise ValueError(op)


def random_mask(shape, density: float, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ------------------------------------------------------------------ inputs and the oracle's histogram
ORACLE_CASES = ("stripes", "noise", "real_256")
ODD_SHAPES = ((3, 30, 30), (2, 33, 47), (1, 5, 4))


@functools.lru_cache(maxsize=None)
def tiles_u8(case: str) -> torch.Tensor:
    if case == "stripes":
        return mn.striped_tiles()
    if case == "noise":
        return mn.noise_tiles()
    if case == "real_256":
        return mn.real_crops(256)
    shape = ODD_SHAPES[int(case.split("_")[1])]
    return synth.noise_u8((shape[0], 3, shape[1], shape[2]), 143)


def all_cases() -> tuple[str, ...]:
    return ORACLE_CASES + tuple(f"odd_{i}" for i in range(len(ODD_SHAPES)))


@functools.lru_cache(maxsize=None)
def oracle_histogram(case: str, dtype_name: str) -> tuple[np.ndarray, np.ndarray]:
    """(below (N, 255), near (N, 255)) int64 per tile: the pixels whose oracle lightness L lies below the cut 255 k / 256, and those within
    L_BAND of it, k = 1..255 (column k - 1).  ``below`` is the running sum of the oracle's histogram, bin floor(L / 255 * 256) clamped."""
    dtype = {"u8": torch.uint8, "f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    lum = mn.lightness(mn.oracle_input(synth.as_dtype(tiles_u8(case), dtype))).astype(np.float64)
    n = lum.shape[0]
    flat = lum.reshape(n, -1)
    bins = np.clip(np.floor(flat / 255.0 * 256.0), 0, 255).astype(np.int64)
    below = np.stack([np.cumsum(np.bincount(row, minlength=256))[:255] for row in bins])
    nearest = np.clip(np.rint(flat / 255.0 * 256.0), 1, 255).astype(np.int64)
    close = np.abs(flat - 255.0 * nearest / 256.0) <= L_BAND
    near = np.stack([np.bincount(nearest[i][close[i]], minlength=256)[1:] for i in range(n)])
    return below.astype(np.int64), near.astype(np.int64)


def oracle_bin_of_grey(level: int) -> int:
    """The oracle's bin of a pixel whose three channels hold the grey level ``level``."""
    lum = float(mn.lightness(np.full((1, 3, 1, 1), level, dtype=np.uint8))[0, 0, 0])
    return min(int(math.floor(lum / 255.0 * 256.0)), 255)
