"""The yardstick of the stain-quantification tests: the binning rule and the fixed-point term of include/stainx_hip.h
(sx_deconv_quantify) restated in numpy.

``histogram_of`` takes float32 concentrations -- what ``sx_deconv_separate`` writes -- and applies the contract to them in float32 /
int64: ``np.floor`` of an exact product with a power of two and ``np.rint`` (round to nearest even) are the same functions as the
kernel's, so the comparison is exact.  ``float64_bins`` / ``sure_and_near`` restate the same rule on the float64 concentrations of
tests/_deconv_numpy.py (imported, unchanged): a pixel whose float64 ``C 2^k`` lies within ``tol 2^k`` of an integer may land in either
of the two bins that meet there, every other pixel's bin is certain."""
from __future__ import annotations

import numpy as np

from tests import _deconv_numpy as dn

F32 = np.float32
F64 = np.float64
BINS = 256
SUM_SCALE = 65536.0      # the sums are fixed point, units of 2^-16
CONC_TOL = 3e-5          # the project's bound on a float32 concentration against float64 (tests/test_deconv_gpu.py)


def bins_of(conc_f32: np.ndarray, k: int, z: int) -> np.ndarray:
    """clamp((int)floor(C 2^k) + z, 0, 255) of finite float32 concentrations, int64."""
    with np.errstate(over="ignore"):
        f = np.floor(np.asarray(conc_f32, dtype=F32) * F32(2.0**k))      # (exact unless it overflows to +-inf, which the clip takes)
    return np.clip(np.clip(f.astype(F64), -1024.0, 1024.0).astype(np.int64) + z, 0, BINS - 1)


def terms_of(conc_f32: np.ndarray) -> np.ndarray:
    """C 2^16 converted to int32, round to nearest even, saturating -- as int64."""
    with np.errstate(over="ignore"):
        t = np.rint(np.asarray(conc_f32, dtype=F32) * F32(SUM_SCALE))
    return np.clip(t.astype(F64), -(2.0**31), 2.0**31 - 1).astype(np.int64)


def histogram_of(conc_f32: np.ndarray, k: int, z: int, keep: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(counts (N, 3, 256), sums (N, 3), pixels (N,))`` int64 of (N, 3, H, W) float32 concentrations: a pixel counts iff its three
    concentrations are finite and (``keep``: (N, H, W) bool) it is kept."""
    c = np.asarray(conc_f32, dtype=F32)
    n = c.shape[0]
    c = c.reshape(n, 3, -1)
    ok = np.isfinite(c).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep).reshape(n, -1).astype(bool)
    counted = np.broadcast_to(ok[:, None, :], c.shape)
    with np.errstate(invalid="ignore"):      # (what is not counted may be anything)
        finite = np.where(counted, c, F32(0.0))
        slot = bins_of(finite, k, z) + (np.arange(n * 3, dtype=np.int64) * BINS).reshape(n, 3, 1)      # one bincount for every (tile, stain)
    counts = np.bincount(slot[counted], minlength=n * 3 * BINS).reshape(n, 3, BINS)
    sums = np.where(counted, terms_of(finite), 0).sum(axis=-1)
    return counts, sums, ok.sum(axis=1).astype(np.int64)


def pooled(counts: np.ndarray, sums: np.ndarray, pixels: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    return counts.sum(axis=0, keepdims=True), sums.sum(axis=0, keepdims=True), pixels.sum(axis=0, keepdims=True)


def concentrations64(images: np.ndarray, basis) -> np.ndarray:
    """(N, 3, H, W) float64 concentrations of the restated contract."""
    return dn.concentrations(images, basis)


def near_edge(conc64: np.ndarray, k: int, tol: float = CONC_TOL) -> np.ndarray:
    """Bool, the shape of ``conc64``: the float64 ``C 2^k`` lies within ``tol 2^k`` of an integer (a bin edge)."""
    scaled = np.asarray(conc64, dtype=F64) * 2.0**k
    return np.abs(scaled - np.rint(scaled)) <= tol * 2.0**k


def near_edge_share(conc64: np.ndarray, k: int, tol: float = CONC_TOL) -> np.ndarray:
    """(N, 3): the share of near-edge values per tile and stain."""
    n = conc64.shape[0]
    return near_edge(conc64, k, tol).reshape(n, 3, -1).mean(axis=-1)


def sure_and_near(conc64: np.ndarray, k: int, z: int, tol: float = CONC_TOL) -> tuple[np.ndarray, np.ndarray]:
    """``(sure, near)``, each (N, 3, 256) int64.  ``sure[b]``: the values whose float64 bin is b and that are not near an edge;
    ``near[b]``: the near-edge values of b's two edges (each such value is listed under both bins that meet at its edge; the end bins,
    which also take what lies beyond the range, list every near-edge value at or beyond their inner edge)."""
    n = conc64.shape[0]
    c = np.asarray(conc64, dtype=F64).reshape(n, 3, -1)
    scaled = c * 2.0**k
    close = near_edge(c, k, tol)
    sure, near = np.zeros((n, 3, BINS), np.int64), np.zeros((n, 3, BINS), np.int64)
    for i in range(n):
        for s in range(3):
            far = ~close[i, s]
            b = np.clip(np.floor(scaled[i, s][far]).astype(np.int64) + z, 0, BINS - 1)
            sure[i, s] = np.bincount(b, minlength=BINS)
            edge = np.rint(scaled[i, s][close[i, s]]).astype(np.int64) + z      # the edge index e: bins e - 1 and e meet there
            near[i, s] = np.bincount(np.clip(edge, 0, BINS - 1), minlength=BINS) + np.bincount(np.clip(edge - 1, 0, BINS - 1), minlength=BINS)
    return sure, near


# ---- the figures, brute force from concentrations (what a user computes from the map today) ----
def positive_fraction(values: np.ndarray, threshold: float) -> float:
    return float((values >= threshold).sum()) / values.size if values.size else 0.0


def h_score(values: np.ndarray, thresholds) -> float:
    t1, t2, t3 = thresholds
    if not values.size:
        return 0.0
    weak, moderate, strong = ((values >= t1) & (values < t2)).sum(), ((values >= t2) & (values < t3)).sum(), (values >= t3).sum()
    return 100.0 * float(weak + 2 * moderate + 3 * strong) / values.size


def quantile_edge(values: np.ndarray, q: float, k: int, z: int) -> float:
    """The lower edge of the bin of the nearest-rank element: rank max(1, ceil(q n)) in ascending order."""
    if not values.size:
        return float("nan")
    rank = max(1, int(np.ceil(q * values.size)))
    element = np.sort(np.asarray(values, dtype=F32))[rank - 1]
    return float(bins_of(np.array([element], dtype=F32), k, z)[0] - z) / 2.0**k
