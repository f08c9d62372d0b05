"""Float64 restatement of the Vahadane estimate (include/stainx_hip.h: sx_vahadane_estimate) for the tests.

Objective: 0.5 |V - W H|^2 + lam |H|_1 over W (3, 2) >= 0 with unit columns and H (2, n) >= 0, V (3, n) the optical density.  One round:
the exact two-variable non-negative lasso per pixel, then one block-coordinate sweep of the dictionary update; exactly ``iterations``
rounds; afterwards the column with the larger red optical density comes first."""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
HE_INIT = np.array([[0.644211, 0.092789], [0.716556, 0.954111], [0.266844, 0.283111]], dtype=np.float64)      # stain_basis("he")'s H and E before normalisation


def real_images() -> np.ndarray:
    """(6, 3, 1024, 1024) uint8: the six real H&E images of the golden set."""
    with np.load(GOLDEN / "g11_real_images.npz", allow_pickle=False) as z:
        return z["images_u8"]


def optical_density(images: np.ndarray) -> np.ndarray:
    """-log((level + 1) / 240) in float64.  uint8: the grey levels; floats: level = 255 x."""
    x = np.asarray(images)
    level = x.astype(np.float64) if x.dtype == np.uint8 else 255.0 * x.astype(np.float64)
    return np.log(240.0) - np.log(level + 1.0)


def normalise_columns(w: np.ndarray) -> np.ndarray:
    w = np.asarray(w, dtype=np.float64).reshape(3, 2).copy()
    nrm = np.sqrt((w * w).sum(axis=0))
    nrm[nrm == 0.0] = 1.0
    return w / nrm


def code(w: np.ndarray, v: np.ndarray, lam: float) -> np.ndarray:
    """The coding step: H (2, n) for W (3, 2) and V (3, n)."""
    g = float(w[:, 0] @ w[:, 1])
    b = w.T @ v - lam
    b1, b2 = b[0], b[1]
    d = 1.0 - g * g
    h = np.zeros_like(b)
    both = np.zeros(b1.shape, dtype=bool)
    if d > 1e-6:
        c1, c2 = (b1 - g * b2) / d, (b2 - g * b1) / d
        both = (c1 > 0.0) & (c2 > 0.0)
        h[0, both], h[1, both] = c1[both], c2[both]
    first = ~both & (b1 > 0.0) & (b2 - g * b1 <= 0.0)
    h[0, first] = b1[first]
    second = ~both & ~first & (b2 > 0.0)
    h[1, second] = b2[second]
    return h


def dictionary_step(w: np.ndarray, v: np.ndarray, h: np.ndarray) -> np.ndarray:
    a, b = h @ h.T, v @ h.T
    w = w.copy()
    for j in range(2):
        if a[j, j] == 0.0:
            continue
        u = np.maximum(w[:, j] + (b[:, j] - w @ a[:, j]) / a[j, j], 0.0)
        nrm = np.sqrt(u @ u)
        if nrm == 0.0:
            continue
        w[:, j] = u / nrm
    return w


def objective(w: np.ndarray, h: np.ndarray, v: np.ndarray, lam: float) -> float:
    r = v - w @ h
    return 0.5 * float((r * r).sum()) + lam * float(h.sum())


def rounds(v: np.ndarray, init: np.ndarray = HE_INIT, lam: float = 0.1, iterations: int = 30) -> np.ndarray:
    """W (3, 2) in float64 after exactly ``iterations`` rounds, before the ordering rule."""
    w = normalise_columns(init)
    for _ in range(iterations):
        w = dictionary_step(w, v, code(w, v, lam))
    return w


def order(w: np.ndarray) -> np.ndarray:
    return w[:, ::-1].copy() if w[0, 0] < w[0, 1] else w


def estimate(images: np.ndarray, mask: np.ndarray | None = None, *, pooled: bool = False, init: np.ndarray = HE_INIT, lam: float = 0.1, iterations: int = 30) -> np.ndarray:
    """(rows, 3, 2) float64: the estimate of every tile of ``images`` (N, 3, H, W), or pooled over the batch; NaN for an empty group.
    ``mask``: (N, H, W), non-zero = in, or None.  ``init``: (3, 2) or one per row."""
    n = images.shape[0]
    od = optical_density(images).reshape(n, 3, -1)
    keep = np.ones((n, od.shape[2]), dtype=bool) if mask is None else np.asarray(mask).reshape(n, -1) != 0
    groups = [np.arange(n)] if pooled else [np.array([t]) for t in range(n)]
    init = np.asarray(init, dtype=np.float64).reshape(-1, 3, 2)
    out = np.full((len(groups), 3, 2), np.nan)
    for r, tiles in enumerate(groups):
        v = np.concatenate([od[t][:, keep[t]] for t in tiles], axis=1)
        if v.shape[1] == 0:
            continue
        out[r] = order(rounds(v, init[r if init.shape[0] > 1 else 0], lam, iterations))
    return out


def angle_degrees(a: np.ndarray, b: np.ndarray) -> float:
    c = float(a @ b) / float(np.sqrt(a @ a) * np.sqrt(b @ b))
    return float(np.degrees(np.arccos(min(1.0, c))))
