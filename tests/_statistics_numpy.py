"""The yardstick of the statistics-space augmentation tests: the moments rule of include/stainx_hip.h (sx_deconv_moments), the draw
formulas of ``StatisticsAugment.sample_targets`` and the factors of ``ColorDeconvolution.match``, restated in numpy.

``moments_of`` takes float32 concentrations -- what ``sx_deconv_separate`` writes -- and applies the contract to them in int64, on the
fixed-point term of tests/_quantify_numpy.py (``terms_of``, imported, unchanged): integers throughout, so the comparison with the
kernel is exact.  ``moments64`` is the same rule on the float64 concentrations of tests/_deconv_numpy.py rounded to float32 -- what the
statistics of a tile are, independent of the kernels' fold."""
from __future__ import annotations

import numpy as np

from tests import _deconv_numpy as dn
from tests import _quantify_numpy as qn

F32 = np.float32
F64 = np.float64
CLAMP = 1 << 22            # |u_s| <= 2^22: a concentration beyond +-64 enters the squares as 64
SQUARE_SHIFT = 8           # (u u) >> 8: units of 2^-24
SQUARE_SCALE = 2.0**24
TINY = np.finfo(F32).tiny


def squares_of(terms: np.ndarray) -> np.ndarray:
    """(u u) >> 8 of int64 terms, u = clamp(t, -2^22, 2^22)."""
    u = np.clip(np.asarray(terms, dtype=np.int64), -CLAMP, CLAMP)
    return (u * u) >> SQUARE_SHIFT


def moments_of(conc_f32: np.ndarray, keep: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(sums (N, 3), squares (N, 3), pixels (N,))`` int64 of (N, 3, H, W) float32 concentrations: a pixel counts iff its three
    concentrations are finite and (``keep``: (N, H, W) bool) it is kept."""
    c = np.asarray(conc_f32, dtype=F32)
    n = c.shape[0]
    c = c.reshape(n, 3, -1)
    ok = np.isfinite(c).all(axis=1)
    if keep is not None:
        ok &= np.asarray(keep).reshape(n, -1).astype(bool)
    counted = np.broadcast_to(ok[:, None, :], c.shape)
    with np.errstate(invalid="ignore"):      # (what is not counted may be anything)
        terms = qn.terms_of(np.where(counted, c, F32(0.0)))
    sums = np.where(counted, terms, 0).sum(axis=-1)
    squares = np.where(counted, squares_of(terms), 0).sum(axis=-1)
    return sums, squares, ok.sum(axis=1).astype(np.int64)


def moments64(images: np.ndarray, basis, keep: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The rule on the restated float64 concentrations (tests/_deconv_numpy.py), rounded to float32."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return moments_of(dn.concentrations(images, basis).astype(F32), keep)


def pooled(sums: np.ndarray, squares: np.ndarray, pixels: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    return sums.sum(axis=0, keepdims=True), squares.sum(axis=0, keepdims=True), pixels.sum(axis=0, keepdims=True)


def mean_std(sums: np.ndarray, squares: np.ndarray, pixels: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``ConcentrationStatistics.mean`` / ``.std`` in float64: NaN where fewer than two pixels were counted."""
    p = np.asarray(pixels, dtype=F64)[:, None]
    some = np.maximum(p, 1.0)
    s = np.asarray(sums, dtype=F64) / qn.SUM_SCALE
    q = np.asarray(squares, dtype=F64) / SQUARE_SCALE
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / some
        std = np.sqrt(np.maximum((q - s * mean) / np.maximum(some - 1.0, 1.0), 0.0))
    none = np.broadcast_to(p < 2.0, mean.shape)
    return np.where(none, np.nan, mean), np.where(none, np.nan, std)


# ---- the draws: z of shape (2, n, 3) from the raw draws of the generator (randn for "normal", rand for the other two) ----
def z_of(kind: str, raw: np.ndarray) -> np.ndarray:
    raw = np.asarray(raw, dtype=F32)
    if kind == "normal":
        return raw
    if kind == "uniform":
        return F32(2.0) * raw - F32(1.0)
    assert kind == "laplace", kind
    u = raw - F32(0.5)
    return -np.sign(u) * np.log(np.maximum(F32(1.0) - F32(2.0) * np.abs(u), TINY))


def targets_of(kind: str, raw: np.ndarray, distribution, spread_scale: float, chosen: np.ndarray | None = None, own=None) -> tuple[np.ndarray, np.ndarray]:
    """``(target_mean, target_std)`` float32 (n, 3): centre + (spread_scale * spread) * z; a tile that is not ``chosen`` gets ``own``'s row."""
    mean_center, mean_spread, std_center, std_spread = (np.asarray(t, dtype=F32) for t in distribution)
    z = z_of(kind, raw)
    mean = mean_center + (F32(spread_scale) * mean_spread) * z[0]
    std = std_center + (F32(spread_scale) * std_spread) * z[1]
    if chosen is not None:
        chosen = np.asarray(chosen, dtype=bool)[:, None]
        mean, std = np.where(chosen, mean, np.asarray(own[0], dtype=F32)), np.where(chosen, std, np.asarray(own[1], dtype=F32))
    return mean.astype(F32), std.astype(F32)


# ---- match: alpha = clamp(target_std / source_std, gain_range), beta = target_mean - alpha source_mean, in float32 ----
def match_factors(source_mean, source_std, target_mean, target_std, n: int, gain_range=(0.1, 2.5)) -> tuple[np.ndarray, np.ndarray]:
    sm, ss, tm, ts = (np.broadcast_to(np.asarray(t, dtype=F32).reshape(-1, 3), (n, 3)) for t in (source_mean, source_std, target_mean, target_std))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = ts / ss
        alpha = np.where(np.isnan(ratio), ratio, np.clip(ratio, F32(gain_range[0]), F32(gain_range[1]))).astype(F32)
        beta = (tm - alpha * sm).astype(F32)
    leave = (np.isnan(sm) | np.isnan(ss) | (ss == 0) | np.isnan(tm) | np.isnan(ts)).any(axis=1, keepdims=True)
    return np.where(leave, F32(1.0), alpha).astype(F32), np.where(leave, F32(0.0), beta).astype(F32)


def fit_distribution(means: np.ndarray, stds: np.ndarray):
    """Centres and unbiased spreads over the rows without a NaN, float64 -> float32."""
    means, stds = np.asarray(means, dtype=F64).reshape(-1, 3), np.asarray(stds, dtype=F64).reshape(-1, 3)
    valid = ~(np.isnan(means).any(axis=1) | np.isnan(stds).any(axis=1))
    means, stds = means[valid], stds[valid]
    return tuple(v.astype(F32) for v in (means.mean(axis=0), means.std(axis=0, ddof=1), stds.mean(axis=0), stds.std(axis=0, ddof=1)))
