"""The tone jitter's pixel rule (include/stainx_hip.h: sx_tone_apply) restated in float64.  numpy only.

What is evaluated are the float32 VALUES the kernel reads -- the row's four floats and the input levels (tests/_hsv_numpy.py:
``input_levels``) -- and the integers of the generator, which are exact: Philox4x32-10 on (pixel index, seed), the uniforms
``(2 (w >> 9) + 1) 2^-24`` and Box-Muller in float64.  ``levels64`` returns the level of every channel on the 0-255 scale BEFORE the output
rule (tests/_hsv_numpy.py: ``to_output`` applies it)."""
from __future__ import annotations

import numpy as np

IDENTITY = (1.0, 0.0, 1.0, 0.0)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """``counter``: (..., 4) and ``key``: (..., 2) unsigned 32-bit words (broadcast against each other) -> (..., 4) uint32 words."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2      # (32 x 32 -> 64 bits: no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> SHIFT32) ^ c1 ^ k0, p1 & MASK32, (p0 >> SHIFT32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(words: np.ndarray) -> np.ndarray:
    """``(2 (w >> 9) + 1) 2^-24`` in float64: an odd integer below 2^24 over 2^24, exact in float32 as well, strictly inside (0, 1)."""
    return (2.0 * (np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0**-24


def normals(seed: int, pixels: np.ndarray) -> np.ndarray:
    """(P, 4) float64 standard normals ``(z_r, z_g, z_b, z_s)`` of the pixel indices ``pixels`` (P,) of a tile with the int64 ``seed``."""
    p = np.asarray(pixels, dtype=np.uint64)
    s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    zero = np.zeros_like(p)
    words = philox4x32_10(np.stack([p & MASK32, p >> SHIFT32, zero, zero], axis=-1), np.array([s & MASK32, (s >> SHIFT32) & MASK32], dtype=np.uint64))
    u = uniform(words)
    rho_a, rho_b = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    angle_a, angle_b = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([rho_a * np.cos(angle_a), rho_a * np.sin(angle_a), rho_b * np.cos(angle_b), rho_b * np.sin(angle_b)], axis=-1)


def row_is_copy(row) -> bool:
    a, b, gamma, sigma = (float(np.float32(v)) for v in row)
    return not (all(np.isfinite(v) for v in (a, b, gamma, sigma)) and gamma > 0.0 and sigma >= 0.0)


def levels64(levels: np.ndarray, row, seed: int | None = None, pixels: np.ndarray | None = None, shared: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """``levels``: (P, 3) float64 input levels (NaN / Inf allowed); ``row``: four numbers, taken as their float32 values; ``seed`` (None: no
    noise) and ``pixels`` (P,): the tile's seed and each pixel's index in its tile.  -> ``(out, copied)``: (P, 3) float64 levels in
    [0, 255] and (P,) bool, the pixels the rule copies (a NaN member, or a row that says "leave this tile")."""
    a, b, gamma, sigma = (float(np.float32(v)) for v in row)
    levels = np.asarray(levels, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        has_nan = np.isnan(levels).any(axis=1)
        x = np.clip(np.where(np.isnan(levels), 0.0, levels), 0.0, 255.0)      # (fmaxf(NaN, 0) = 0: the background rule's clamp)
        copied = has_nan | row_is_copy(row)
        if row_is_copy(row):
            return x, copied
        t = np.clip(a * x + 255.0 * b, 0.0, 255.0)
        if gamma != 1.0:
            t = np.where(t > 0.0, 255.0 * np.power(t / 255.0, gamma), 0.0)
        if seed is not None and sigma > 0.0:
            z = normals(seed, pixels)
            zc = np.repeat(z[:, 3:4], 3, axis=1) if shared else z[:, :3]
            t = np.clip(t + 255.0 * sigma * zc, 0.0, 255.0)
    return np.where(copied[:, None], x, t), copied
