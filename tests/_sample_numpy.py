"""The rule of ``stainx_amd.sample_pixels`` restated in numpy and Python integers, straight from its statement (include/stainx_hip.h, DESIGN.md
5j): a loop over slots, no sort, no search.  What the GPU tests compare with bit for bit, and what tools/sample_deviation.py samples with."""
from __future__ import annotations

import numpy as np


def slot_ranks(n: int, k: int, offset: int) -> list[int]:
    """The rank each of the first ``min(n, k)`` slots holds: the identity for ``n <= k``, else ``(j * n + o) // k`` with ``o = offset % n``."""
    if n <= k:
        return list(range(n))
    o = offset % n
    return [(j * n + o) // k for j in range(k)]


def pixel_side(r: int, n: int, k: int, offset: int) -> int | None:
    """The pixel-side test of DESIGN.md 5j for ``n > k``: the slot that takes the pixel of rank ``r``, or None.  ``j0 = ceil((r k - o) / n)`` clamped at
    0 is the first slot whose rank is at least r; r is taken iff ``j0 < k`` and that slot's rank is r."""
    o = offset % n
    j0 = max(0, -((o - r * k) // n))      # ceil((r k - o) / n) in integers
    return j0 if j0 < k and (j0 * n + o) // k == r else None


def first_slot(rank: int, n: int, k: int, offset: int) -> int:
    """J(R) of DESIGN.md 5j for ``n > k``: the first slot whose rank is at least R (k when there is none below k: J(n) = k)."""
    o = offset % n
    return max(0, -((o - rank * k) // n))


def sample_pixels(images: np.ndarray, size: tuple[int, int], mask: np.ndarray | None = None, pooled: bool = False, offset: int = 0):
    """``images``: (N, 3, H, W) of any element type; ``mask``: (N, H, W), non-zero = in, or None.  Returns ``(pixels (G, 3, h, w), valid (G, h, w) uint8,
    taken (G,) int32, population (G,) int64)``; the pixels are moved with their bits (the arrays are handled through integer views)."""
    n_tiles, _, height, width = images.shape
    h, w = size
    k = h * w
    bits = images.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[images.dtype.itemsize])
    flat = bits.reshape(n_tiles, 3, height * width)
    inside = np.ones((n_tiles, height * width), dtype=bool) if mask is None else np.asarray(mask).reshape(n_tiles, height * width) != 0
    groups = [list(range(n_tiles))] if pooled else [[t] for t in range(n_tiles)]
    pixels = np.zeros((len(groups), 3, k), dtype=bits.dtype)
    valid = np.zeros((len(groups), k), dtype=np.uint8)
    taken = np.zeros((len(groups),), dtype=np.int32)
    population = np.zeros((len(groups),), dtype=np.int64)
    for g, tiles in enumerate(groups):
        ranked = np.concatenate([flat[t][:, inside[t]] for t in tiles], axis=1)      # (3, n): the population in rank order
        n = ranked.shape[1]
        for j, r in enumerate(slot_ranks(n, k, offset)):
            pixels[g, :, j] = ranked[:, r]
            valid[g, j] = 1
        taken[g] = min(n, k)
        population[g] = n
    return pixels.reshape(len(groups), 3, h, w).view(images.dtype), valid.reshape(len(groups), h, w), taken, population
