"""The elastic warp's rule (stainx_amd/csrc/elastic.hpp, include/stainx_hip.h: sx_elastic_warp) restated in float64, on
tests/_warp_numpy.py -- its taps, border, ``fill`` and output rule.  numpy only.

What is evaluated are the float32 VALUES the kernel reads -- the tile's six float32, the grid's float32 control displacements and the stored
elements --, with ``t``, the spline weights, the two four-term sums, the coordinates, the fractions and the interpolation in float64: the
restatement differs from the kernel by the kernel's own float32 arithmetic and nothing else.  ``nearest`` is the exception, as in
``_warp_numpy``: it takes the FLOAT32 coordinates (``coords32``: the kernel's operations one by one) and rounds them as the kernel does.

THE BAND (``coordinate_band``) is derived from the rule's operation count, not fitted to the kernel.  With u = 2^-24, the unit roundoff of
float32, and M = max |P| over the plane's control displacements, per axis:
  the affine term   2^-23 S (``_warp_numpy.coordinate_slack``: two roundings of numbers <= S).
  the weights       t is one division: off by <= u.  B0 and B3: three products and the factor float32(1/6) on a value <= 1/6, and
                    |B'| <= 1/2: <= 1.5 u each.  B1 = fmaf(t t, fmaf(3, t, -6), 4) / 6: the inner term (<= 6 in magnitude) is off by
                    <= 6 u, t t by <= u (times 6), the outer sum (<= 4) rounds by <= 4 u: 16 u, a sixth of it 2.7 u, the last product
                    and the factor 1.3 u, |B1'| <= 2/3: <= 4.7 u.  B2 likewise <= 4 u.  The four together: <= 12 u.
  the x pass        12 u M from the weights, four roundings of partial sums that are <= M (the weights are >= 0 and sum to 1): 16 u M.
  the y pass        16 u M carried (weights sum to 1), 12 u M from its own weights, 4 u M from its roundings: 32 u M -- taken as
                    ELASTIC_OPS = 40 to cover the second-order terms that the count leaves out.
  the final add     s + d rounds by <= u (S + M); nearest's s + 0.5 by as much again: 2^-23 (S + M).
The value moves by at most the largest difference of neighbours (255 levels, 1.0 on [0, 1]) per pixel of coordinate error and axis;
``value_band`` adds tests/test_warp_gpu.py's terms: 0.5 + 1e-3 levels for uint8 output, 1e-6 + the half unit of the float type."""
from __future__ import annotations

import numpy as np

from tests import _warp_numpy as wn

ELASTIC_OPS = 40.0
SIXTH32 = np.float32(1.0) / np.float32(6.0)


def grid_shape(out_size, cell: int) -> tuple[int, int]:
    return (out_size[0] - 1) // cell + 4, (out_size[1] - 1) // cell + 4


def weights(t: np.ndarray) -> np.ndarray:
    """(4, ...) float64: the uniform cubic B-spline's four weights of ``t`` in [0, 1)."""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([(1.0 - t) ** 3 / 6.0, (3.0 * t**3 - 6.0 * t**2 + 4.0) / 6.0, (-3.0 * t**3 + 3.0 * t**2 + 3.0 * t + 1.0) / 6.0, t**3 / 6.0])


def _cells(n: int, cell: int) -> tuple[np.ndarray, np.ndarray]:
    x = np.arange(n, dtype=np.int64)
    j = x // cell
    return j, (x - j * cell).astype(np.float64) / float(cell)


def displacement(grid, out_size, cell: int) -> tuple[np.ndarray, np.ndarray]:
    """(dx, dy), each (OH, OW) float64, of the float32 grid (2, GH, GW): ``sum_l B_l(ty) sum_k B_k(tx) P[jy + l][jx + k]``."""
    oh, ow = out_size
    grid = np.asarray(grid, dtype=np.float32).astype(np.float64)
    assert grid.shape == (2, *grid_shape(out_size, cell)), (grid.shape, out_size, cell)
    jx, tx = _cells(ow, cell)
    jy, ty = _cells(oh, cell)
    wx, wy = weights(tx), weights(ty)
    with np.errstate(invalid="ignore", over="ignore"):
        across = sum(wx[k][None, None, :] * grid[:, :, jx + k] for k in range(4))      # (2, GH, OW): the x pass
        field = sum(wy[l][None, :, None] * across[:, jy + l, :] for l in range(4))     # (2, OH, OW): the y pass
    return field[0], field[1]


def coords(row, grid, out_size, cell: int) -> tuple[np.ndarray, np.ndarray]:
    """(sx, sy) float64 of the row IN USE (finite) and the grid."""
    ax, ay = wn.coords(row, *out_size)
    dx, dy = displacement(grid, out_size, cell)
    with np.errstate(invalid="ignore", over="ignore"):
        return ax + dx, ay + dy


def _mul32(a, b) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, dtype=np.float32) * np.asarray(b, dtype=np.float32)).astype(np.float32)


def weights32(t: np.ndarray) -> list:
    """``elastic_weights`` operation by operation in float32."""
    t = np.asarray(t, dtype=np.float32)
    one = np.ones_like(t)
    u = (one - t).astype(np.float32)
    b0 = _mul32(_mul32(_mul32(u, u), u), SIXTH32)
    b1 = _mul32(wn._fma32(_mul32(t, t), wn._fma32(np.float32(3.0), t, np.full_like(t, -6.0)), np.full_like(t, 4.0)), SIXTH32)
    b2 = _mul32(wn._fma32(t, wn._fma32(t, wn._fma32(np.float32(-3.0), t, np.full_like(t, 3.0)), np.full_like(t, 3.0)), one), SIXTH32)
    b3 = _mul32(_mul32(_mul32(t, t), t), SIXTH32)
    return [b0, b1, b2, b3]


def _sum32(w: list, p: list) -> np.ndarray:
    """``elastic_sum``: fmaf(w3, p3, fmaf(w2, p2, fmaf(w1, p1, w0 p0)))."""
    acc = _mul32(w[0], p[0])
    for k in (1, 2, 3):
        acc = wn._fma32(w[k], np.asarray(p[k], dtype=np.float32), acc)
    return acc


def displacement32(grid, out_size, cell: int) -> tuple[np.ndarray, np.ndarray]:
    """(dx, dy) float32 as the kernel evaluates them."""
    oh, ow = out_size
    grid = np.asarray(grid, dtype=np.float32)
    jx, tx = _cells(ow, cell)
    jy, ty = _cells(oh, cell)
    tx32, ty32 = (np.arange(ow) - jx * cell).astype(np.float32) / np.float32(cell), (np.arange(oh) - jy * cell).astype(np.float32) / np.float32(cell)
    wx, wy = weights32(tx32.astype(np.float32)), weights32(ty32.astype(np.float32))
    across = _sum32([w[None, None, :] for w in wx], [grid[:, :, jx + k] for k in range(4)])
    field = _sum32([w[None, :, None] for w in wy], [across[:, jy + l, :] for l in range(4)])
    return field[0], field[1]


def coords32(row, grid, out_size, cell: int) -> tuple[np.ndarray, np.ndarray]:
    ax, ay = wn.coords32(row, *out_size)
    dx, dy = displacement32(grid, out_size, cell)
    with np.errstate(invalid="ignore", over="ignore"):
        return (ax + dx).astype(np.float32), (ay + dy).astype(np.float32)


def bilinear_at(values: np.ndarray, sx: np.ndarray, sy: np.ndarray, border: str, fill: float) -> np.ndarray:
    """``_warp_numpy.warp64``'s bilinear rule at given float64 coordinates: the limit test, the taps through the border rule, the three
    steps, the stored element where both fractions are 0."""
    ok = wn.coord_ok(sx) & wn.coord_ok(sy)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        v00, v01 = wn._tap(values, yi, xi, border, fill), wn._tap(values, yi, xi + 1, border, fill)
        v10, v11 = wn._tap(values, yi + 1, xi, border, fill), wn._tap(values, yi + 1, xi + 1, border, fill)
        top = v00 + fx * (v01 - v00)
        bot = v10 + fx * (v11 - v10)
        out = top + fy * (bot - top)
        out = np.where((fx == 0.0) & (fy == 0.0), v00, out)
    return np.where(ok, out, fill)


def nearest_at(values: np.ndarray, sx32: np.ndarray, sy32: np.ndarray, border: str, fill) -> np.ndarray:
    """``_warp_numpy.nearest`` at given FLOAT32 coordinates."""
    ok = wn.coord_ok(sx32) & wn.coord_ok(sy32)
    half = np.float32(0.5)
    xi = np.floor(np.where(ok, sx32, np.float32(0)) + half).astype(np.int64)
    yi = np.floor(np.where(ok, sy32, np.float32(0)) + half).astype(np.int64)
    return np.where(ok, wn._tap(values, yi, xi, border, fill), np.asarray(fill, dtype=values.dtype))


def warp64(values: np.ndarray, row, grid, cell: int, out_size=None, *, interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0) -> np.ndarray:
    """``values``: (..., H, W); ``row``: six numbers; ``grid``: (2, GH, GW) -> (..., OH, OW) before the output rule.  A row with a NaN or an
    infinity leaves the tile as ``_warp_numpy.warp64`` does: the grid is not read."""
    values = np.asarray(values)
    h, w = values.shape[-2:]
    out_size = tuple(out_size or (h, w))
    if not np.isfinite(np.asarray(row, dtype=np.float32)).all():
        return wn.warp64(values, row, out_size, interpolation=interpolation, border=border, fill=fill)
    if interpolation == "nearest":
        return nearest_at(values, *coords32(row, grid, out_size, cell), border, fill)
    return bilinear_at(values.astype(np.float64), *coords(row, grid, out_size, cell), border, fill)


def grid_max(grid) -> tuple[float, float]:
    """(max |P0|, max |P1|) over the finite control displacements."""
    g = np.abs(np.asarray(grid, dtype=np.float32).astype(np.float64))
    g = np.where(np.isfinite(g), g, 0.0)
    return float(g[0].max()), float(g[1].max())


def coordinate_band(row, grid, out_size) -> tuple[float, float]:
    """(Ex, Ey): how far a float32 coordinate of the kernel may lie from the float64 one (the module's docstring); ``row`` is the row in use."""
    s_x, s_y = wn.coordinate_slack(row, *out_size)
    m_x, m_y = grid_max(grid)
    return tuple(2.0**-23 * s + ELASTIC_OPS * 2.0**-24 * m + 2.0**-23 * (s + m) for s, m in ((s_x, m_x), (s_y, m_y)))


def value_band(row, grid, out_size, levels: bool, half_ulp: float = 0.0) -> float:
    """The bilinear band of a tile: levels for uint8 tiles (rounded to a level), [0, 1] for float tiles of the given half unit at 1."""
    e_x, e_y = coordinate_band(row, grid, out_size)
    return 0.5 + 255.0 * (e_x + e_y) + 1e-3 if levels else (e_x + e_y) + 1e-6 + half_ulp


def test_grids(out_size, cell: int, magnitudes=(1.0, 2.0, 3.0), seed: int = 0) -> np.ndarray:
    """(len(magnitudes), 2, GH, GW) float32: seeded normal control displacements, one standard deviation per tile."""
    gh, gw = grid_shape(out_size, cell)
    rng = np.random.default_rng(7919 * cell + 31 * out_size[0] + out_size[1] + seed)
    return (rng.standard_normal((len(magnitudes), 2, gh, gw)) * np.asarray(magnitudes, dtype=np.float64)[:, None, None, None]).astype(np.float32)


test_grids.__test__ = False      # (a helper, not a test)
