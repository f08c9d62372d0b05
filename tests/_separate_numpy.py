"""The yardstick of the separation tests with a given source basis and under tissue masks: stain separation restated from the CPU
oracle's own functions (oracle/stain_oracle.py, imported and unchanged).  Concentrations: ``C = pinv(HE) OD`` as
``so.macenko_tile_params`` forms it (``so.concentrations``: the least-squares solution), scaled by ``tmc / maxC`` with a reference; stain
image i: ``240 exp(-SM[:, i] C'_i)`` with the reference's stain matrix, or the source basis itself without one -- float32 levels on the
0-255 scale BEFORE the clamp and cast.  A masked-out pixel, and every pixel of a tile whose source row holds a NaN, holds no stain:
concentrations 0, both images the level of zero concentration, 240.  What lies under masked-out pixels is never read."""
from __future__ import annotations

import numpy as np

from oracle import stain_oracle as so

F32 = np.float32


def rows_for(rows: np.ndarray | None, n: int, tail: tuple) -> np.ndarray | None:
    """Source rows (one row, or one per tile) broadcast to ``n`` tiles."""
    if rows is None:
        return None
    rows = np.asarray(rows, dtype=F32).reshape((-1,) + tail)
    assert rows.shape[0] in (1, n), rows.shape
    return np.broadcast_to(rows, (n,) + tail)


def separate(images: np.ndarray, mask: np.ndarray, he, max_c=None, reference=None) -> tuple[np.ndarray, np.ndarray]:
    """``images`` (N, 3, H, W) uint8 / float32, ``mask`` (N, H, W) bool, ``he`` (N or 1, 3, 2) and ``max_c`` (N or 1, 2) the source rows
    (``max_c`` is not read without a reference), ``reference`` None (own basis) or ``(stain_matrix (3, 2), target_max_conc (2,))``.
    Returns ``(concentrations (N, 2, H, W), levels (2, N, 3, H, W))`` float32: the H images, then the E images, un-clamped."""
    n, _, h, w = images.shape
    he = rows_for(he, n, (3, 2))
    max_c = rows_for(max_c, n, (2,))
    conc = np.zeros((n, 2, h, w), dtype=F32)
    levels = np.full((2, n, 3, h, w), so.IO, dtype=F32)
    for i in range(n):
        inside = mask[i].reshape(-1)
        row_is_nan = np.isnan(he[i]).any() or (reference is not None and np.isnan(max_c[i]).any())
        if row_is_nan or not inside.any():
            continue
        # (only the masked-in pixels are read: whatever lies under the mask cannot matter)
        od = so.optical_density(so.to_unit_float(np.ascontiguousarray(images[i].reshape(3, -1)[:, inside])))
        c = so.concentrations(he[i], od)
        basis = he[i]
        if reference is not None:
            sm, tmc = np.asarray(reference[0], dtype=F32), np.asarray(reference[1], dtype=F32).reshape(-1)
            c = (c * (tmc / max_c[i])[:, None]).astype(F32)
            basis = sm
        conc[i].reshape(2, -1)[:, inside] = c
        for s in range(2):
            levels[s, i].reshape(3, -1)[:, inside] = so.IO * np.exp(-np.outer(basis[:, s], c[s]).astype(F32))
    return conc, levels


def near_integer_share(levels: np.ndarray, where: np.ndarray, tol: float) -> float:
    """The share of the selected levels within ``tol`` of an integer: where a uint8 cast may land on either side."""
    picked = levels[where]
    return float((np.abs(picked - np.rint(picked)) <= F32(tol)).mean()) if picked.size else 0.0
