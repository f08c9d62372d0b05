"""The Gaussian blur's rule (stainx_amd/csrc/blur.hpp, include/stainx_hip.h: sx_gaussian_blur) restated in float64.  numpy only.

What is evaluated are the float32 VALUES the kernel reads -- the tile's float32 sigma and the stored elements (a uint8 byte as its level, a
float element as it is) -- so the restatement differs from the kernel by the kernel's own float32 arithmetic and nothing else.  The radius
is evaluated on the float32 sigma with the sum 4 sigma + 0.5 taken exactly, as the kernel evaluates it.  ``blur64`` returns the value of
every element BEFORE the output rule; ``to_output`` applies the output rule (8-bit levels rounded to nearest, the casts, the / 255)."""
from __future__ import annotations

import numpy as np
import torch

MAX_SIGMA = 4.0
MAX_RADIUS = 16


def radius(sigma) -> int:
    """R of a sigma's float32 value: 0 for a sigma that copies its tile (NaN, infinite, <= 0, below 0.125)."""
    s = np.float32(sigma)
    if not (np.isfinite(s) and s > 0):
        return 0
    s = min(s, np.float32(MAX_SIGMA))
    return min(int(4.0 * float(s) + 0.5), MAX_RADIUS)      # (the sum of the float32 sigma taken exactly, as the kernel takes it)


def taps(sigma) -> np.ndarray:
    """The 2 R + 1 float64 taps of the float32 value of ``sigma`` (clamped to 4), R >= 1."""
    s = float(min(np.float32(sigma), np.float32(MAX_SIGMA)))
    r = radius(sigma)
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * s * s))
    return w / w.sum()


def fold(q: np.ndarray, n: int) -> np.ndarray:
    """Coordinates reflected into 0..n-1 without repeating the edge, folded as often as needed: period 2 (n - 1); n = 1 maps to 0."""
    q = np.asarray(q, dtype=np.int64)
    if n == 1:
        return np.zeros_like(q)
    period = 2 * (n - 1)
    m = np.mod(q, period)
    return np.where(m >= n, period - m, m)


def filter_axis(x: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    r = (len(w) - 1) // 2
    n = x.shape[axis]
    out = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-r, r + 1):
            out = out + w[k + r] * np.take(x, fold(np.arange(n) + k, n), axis=axis)
    return out


def blur64(values: np.ndarray, sigma) -> np.ndarray:
    """``values``: (..., H, W) float64 -- every leading axis a plane of its own; ``sigma``: one number, taken as its float32 value.
    -> the filtered planes, rows (the last axis) first, then columns; the planes themselves where the sigma copies."""
    values = np.asarray(values, dtype=np.float64)
    if radius(sigma) == 0:
        return values.copy()
    w = taps(sigma)
    return filter_axis(filter_axis(values, w, -1), w, -2)


def input_values(images: torch.Tensor) -> np.ndarray:
    """Elements of any of the five types -> float64: the byte, or the element's value (bf16 / f16 / f32 -> f64 is exact)."""
    return images.to(torch.float64).numpy()


def to_output(value: np.ndarray, in_dtype: torch.dtype, out_dtype: torch.dtype, unit: bool) -> torch.Tensor:
    """The output rule on float64 values: a uint8 tile's level is rounded to the nearest 8-bit level (ties to even) and then cast (and
    divided by 255 in float32); a float tile's value is rounded to the tile's type, and with ``unit`` divided by 255 in float32 and
    rounded again."""
    if in_dtype == torch.uint8:
        q = np.rint(value)
        if out_dtype == torch.uint8:
            return torch.from_numpy(q.astype(np.uint8))
        t = torch.from_numpy(q.astype(np.float32))
        return (t / 255.0).to(out_dtype) if unit else t.to(out_dtype)
    t = torch.from_numpy(value).to(torch.float32).to(in_dtype)
    if not unit:
        return t
    return t / 255.0 if in_dtype == torch.float64 else (t.to(torch.float32) / 255.0).to(in_dtype)
