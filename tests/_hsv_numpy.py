"""The HSV jitter's pixel rule (include/stainx_hip.h: sx_hsv_apply) restated in float64.  numpy only.

What is evaluated are the float32 VALUES the kernel reads -- the row's five floats and the input elements (uint8: the byte as its
level; floats: the element's value, its level 255 x taken in float64) -- so the restatement differs from the kernel by the kernel's own
float32 arithmetic and nothing else.  ``levels64`` returns the level of every channel on the 0-255 scale BEFORE the output rule,
``to_output`` applies the output rule (8-bit levels rounded to nearest, the casts, the / 255)."""
from __future__ import annotations

import numpy as np
import torch

IDENTITY = (0.0, 1.0, 0.0, 1.0, 0.0)
# the fixed rows of the GPU comparison: mild; strong with both clamps active; dh = 0.5 with a_s = 0.3; dh = 0.999 (wraps from every sector)
ROWS = ((0.05, 1.1, -0.03, 0.95, 0.02), (-0.37, 1.8, 0.2, 1.2, -0.1), (0.5, 0.3, 0.0, 1.0, 0.0), (0.999, 1.0, 0.0, 1.0, 0.0))


def input_levels(pixels: torch.Tensor) -> np.ndarray:
    """(..., 3) elements of any of the five types -> float64 levels: the byte, or 255 times the element's value (bf16 / f16 / f32 -> f64 is exact)."""
    if pixels.dtype == torch.uint8:
        return pixels.numpy().astype(np.float64)
    return pixels.to(torch.float64).numpy() * 255.0


def levels64(levels: np.ndarray, row) -> tuple[np.ndarray, np.ndarray]:
    """``levels``: (P, 3) float64 input levels (NaN / Inf allowed); ``row``: five numbers, taken as their float32 values.
    -> ``(out, copied)``: (P, 3) float64 levels in [0, 255] and (P,) bool, the pixels the rule copies (a NaN member, or a non-finite row)."""
    dh, a_s, b_s, a_v, b_v = (float(np.float32(v)) for v in row)
    levels = np.asarray(levels, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        has_nan = np.isnan(levels).any(axis=1)
        clamped = np.clip(np.where(np.isnan(levels), 0.0, levels), 0.0, 255.0)      # (fmaxf(NaN, 0) = 0: the background rule's clamp)
        r, g, b = clamped[:, 0], clamped[:, 1], clamped[:, 2]
        hi, lo = clamped.max(axis=1), clamped.min(axis=1)
        c = hi - lo
        safe_c, safe_hi = np.where(c > 0.0, c, 1.0), np.where(hi > 0.0, hi, 1.0)
        s = np.where(hi > 0.0, c / safe_hi, 0.0)
        first = (g - b) / safe_c
        h6 = np.where(c == 0.0, 0.0, np.where(hi == r, np.where(first < 0.0, first + 6.0, first), np.where(hi == g, 2.0 + (b - r) / safe_c, 4.0 + (r - g) / safe_c)))
        x = h6 + 6.0 * dh
        h = x - 6.0 * np.floor(x / 6.0)
        s2 = np.clip(a_s * s + b_s, 0.0, 1.0)
        v2 = 255.0 * np.clip(a_v * (hi / 255.0) + b_v, 0.0, 1.0)
        out = np.empty_like(clamped)
        for ch, n in enumerate((5.0, 3.0, 1.0)):
            k = h + n
            k = np.where(k >= 6.0, k - 6.0, k)
            t = np.clip(np.minimum(k, 4.0 - k), 0.0, 1.0)
            out[:, ch] = v2 - v2 * s2 * t
    copied = has_nan | (not all(np.isfinite(v) for v in (dh, a_s, b_s, a_v, b_v)))
    return np.where(copied[:, None], clamped, out), copied


def to_output(level: np.ndarray, in_dtype: torch.dtype, out_dtype: torch.dtype, unit: bool) -> torch.Tensor:
    """The output rule on float64 levels in [0, 255]: a uint8 tile's level is rounded to the nearest 8-bit level (ties to even) and
    then cast (and divided by 255 in float32); a float tile's level is rounded to the tile's type, and with ``unit`` divided by 255 in
    float32 and rounded again."""
    if in_dtype == torch.uint8:
        q = np.rint(level)
        if out_dtype == torch.uint8:
            return torch.from_numpy(q.astype(np.uint8))
        t = torch.from_numpy(q.astype(np.float32))
        return (t / 255.0).to(out_dtype) if unit else t.to(out_dtype)
    t = torch.from_numpy(level).to(torch.float32).to(in_dtype)      # (a float64 tile holds the float32 level)
    if not unit:
        return t
    return t / 255.0 if in_dtype == torch.float64 else (t.to(torch.float32) / 255.0).to(in_dtype)


def float32_emulation(levels: np.ndarray, row) -> np.ndarray:
    """The rule in numpy float32, operation by operation with correctly rounded divisions: the
    kernel's reciprocals may differ from it by a few units in the last place.  Finite rows, no NaN members."""
    f = np.float32
    dh, a_s, b_s, a_v, b_v = (f(v) for v in row)
    x = np.clip(np.asarray(levels, dtype=np.float32), f(0), f(255))
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    hi, lo = x.max(axis=1), x.min(axis=1)
    c = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        safe_c, safe_hi = np.where(c > 0, c, f(1)), np.where(hi > 0, hi, f(1))
        s = np.where(hi > 0, c / safe_hi, f(0))
        first = (g - b) / safe_c
        h6 = np.where(c == 0, f(0), np.where(hi == r, np.where(first < 0, first + f(6), first), np.where(hi == g, f(2) + (b - r) / safe_c, f(4) + (r - g) / safe_c))).astype(f)
        xh = h6 + f(6) * dh
        h = xh - f(6) * np.floor(xh / f(6))
        s2 = np.clip(a_s * s + b_s, f(0), f(1))
        v2 = f(255) * np.clip(a_v * (hi / f(255)) + b_v, f(0), f(1))
        out = np.empty_like(x)
        for ch, n in enumerate((f(5), f(3), f(1))):
            k = h + n
            k = np.where(k >= f(6), k - f(6), k)
            t = np.clip(np.minimum(k, f(4) - k), f(0), f(1))
            out[:, ch] = v2 - v2 * s2 * t
    return out
