"""The yardstick of the colour-deconvolution tests: the contract of include/stainx_hip.h (sx_deconv_*) restated in float64, independent
of the kernels' fold.  The optical density comes from the CPU oracle's own functions (``so.to_unit_float`` / ``so.optical_density``,
imported and unchanged), the inverse from ``np.linalg.inv``, the reconstruction is a plain ``exp``:
    C = inverse(basis) OD,   C' = alpha * C + beta,   OD' = B_out C',   level = 240 exp(-OD')
Levels are float32 on the 0-255 scale BEFORE the clamp and the cast, as tests/_separate_numpy.py returns them.  A masked-out pixel,
and every pixel of a tile whose basis (or target) row holds a NaN, is copied: its input level (the byte; x * 255 in float32)."""
from __future__ import annotations

import numpy as np

from oracle import stain_oracle as so

F32 = np.float32
F64 = np.float64

ALPHA = (1.15, 0.9, 1.05)      # the factors of the uint8 cases: the input condition of tests/test_deconv_cpu.py holds for them
BETA = (0.02, -0.03, 0.01)


def uint8_apply_cases(x):
    """The (name, tiles, bases) uint8 cases of the apply tests against the restatement, cut from the six 256 x 256 real crops ``x`` (numpy or
    torch, (6, 3, 256, 256)): the crops themselves, 160 x 112 (more than one work item of the uint8 -> uint8 apply, the last one partial)
    and two odd sizes (the scalar path: one work item, and two with a partial last one).  tests/test_deconv_cpu.py asserts their
    near-integer shares, tests/test_deconv_gpu.py runs them under the full uint8 rule."""
    names = ("hed", "he", "hdab")
    return [("real", x, names), ("160x112", x[:2, :, :160, :112], ("hdab",)), ("33x37", x[:3, :, 11:44, 5:42], ("hdab",)), ("67x65", x[:2, :, 11:78, 5:70], ("hdab",))]


def uint8_separate_cases(x):
    """The same for the stain images of separate: three real crops with every named basis, an odd size and a size with partial work items."""
    return [("real", x[:3], ("hed", "he", "hdab")), ("33x37", x[:3, :, 7:40, 9:46], ("hed",)), ("96x84", x[:3, :, 7:103, 9:93], ("hed",))]


def rows_for(rows, n: int, tail: tuple, dtype=F32):
    """Rows (one, or one per tile) broadcast to ``n`` tiles; None stays None."""
    if rows is None:
        return None
    rows = np.asarray(rows, dtype=dtype).reshape((-1,) + tail)
    assert rows.shape[0] in (1, n), rows.shape
    return np.broadcast_to(rows, (n,) + tail)


def optical_density(images: np.ndarray) -> np.ndarray:
    """(N, 3, H, W) uint8 / float -> (N, 3, P) float64: the oracle's float32 unit value and operation order, carried out in float64."""
    n = images.shape[0]
    unit = so.to_unit_float(np.ascontiguousarray(images)).reshape(n, 3, -1)
    return so.optical_density(unit.astype(F64))


def input_levels(images: np.ndarray) -> np.ndarray:
    """The level of every input element on the 0-255 scale (what a masked-out pixel is copied from), float32."""
    return images.astype(F32) if images.dtype == np.uint8 else images.astype(F32) * F32(255.0)


def concentrations(images: np.ndarray, basis) -> np.ndarray:
    """(N, 3, H, W) float64: C = inverse(basis) OD per tile."""
    n, _, h, w = images.shape
    basis = rows_for(basis, n, (3, 3))
    od = optical_density(images)
    return np.stack([np.linalg.inv(basis[i].astype(F64)) @ od[i] for i in range(n)]).reshape(n, 3, h, w)


def combine(conc: np.ndarray, basis, dtype=F32) -> np.ndarray:
    """(N, 3, H, W) concentrations -> un-clamped levels 240 exp(-basis C)."""
    n, _, h, w = conc.shape
    basis = rows_for(basis, n, (3, 3))
    c = np.asarray(conc, dtype=F64).reshape(n, 3, -1)
    out = np.stack([F64(so.IO) * np.exp(-(basis[i].astype(F64) @ c[i])) for i in range(n)])
    return out.reshape(n, 3, h, w).astype(dtype)


def apply(images: np.ndarray, basis, target=None, alpha=None, beta=None, mask=None, dtype=F32) -> np.ndarray:
    """Un-clamped levels (N, 3, H, W) of sx_deconv_apply / _masked.  ``alpha`` / ``beta``: None or (N or 1, 3); ``mask``: None or (N, H, W)
    bool -- masked-out pixels, and tiles with a NaN in their rows, hold the input's level."""
    n, _, h, w = images.shape
    b = rows_for(basis, n, (3, 3))
    t = b if target is None else rows_for(target, n, (3, 3))
    al = np.ones((n, 3), F64) if alpha is None else rows_for(alpha, n, (3,), F64)
    be = np.zeros((n, 3), F64) if beta is None else rows_for(beta, n, (3,), F64)
    out = np.empty((n, 3, h, w), dtype=F64)
    copied = input_levels(images).astype(F64)
    for i in range(n):
        if np.isnan(b[i]).any() or np.isnan(t[i]).any():
            out[i] = copied[i]
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):      # (what lies under a mask may be anything)
            c = np.linalg.inv(b[i].astype(F64)) @ optical_density(images[i : i + 1])[0]
            c = al[i][:, None] * c + be[i][:, None]
            out[i] = (F64(so.IO) * np.exp(-(t[i].astype(F64) @ c))).reshape(3, h, w)
        if mask is not None:
            keep = np.broadcast_to(mask[i][None], (3, h, w))
            out[i] = np.where(keep, out[i], copied[i])
    return out.astype(dtype)


def stain_images(images: np.ndarray, basis, dtype=F32) -> np.ndarray:
    """(3, N, 3, H, W) un-clamped levels: image i is 240 exp(-basis[:, i] C_i)."""
    n, _, h, w = images.shape
    b = rows_for(basis, n, (3, 3))
    c = concentrations(images, basis).reshape(n, 3, -1)
    out = np.empty((3, n, 3, h * w), dtype=F64)
    for s in range(3):
        for i in range(n):
            out[s, i] = F64(so.IO) * np.exp(-np.outer(b[i][:, s].astype(F64), c[i, s]))
    return out.reshape(3, n, 3, h, w).astype(dtype)


def near_integer_share(levels: np.ndarray, tol: float) -> float:
    """The share of levels within ``tol`` of an integer: where a uint8 cast may land on either side."""
    return float((np.abs(levels - np.rint(levels)) <= F32(tol)).mean()) if levels.size else 0.0


def complement(he: np.ndarray) -> np.ndarray:
    """(..., 3, 2) -> (..., 3, 3): the third column the normalised cross product (HistomicsTK's complement_stain_matrix), float64."""
    he = np.asarray(he, dtype=F64)
    third = np.cross(he[..., 0], he[..., 1])
    third = third / np.linalg.norm(third, axis=-1, keepdims=True)
    return np.concatenate([he, third[..., None]], axis=-1)
