"""The affine warp's rule (stainx_amd/csrc/warp.hpp, include/stainx_hip.h: sx_affine_warp) restated in float64.  numpy only.

What is evaluated are the float32 VALUES the kernel reads -- the tile's six float32 and the stored elements (a uint8 byte as its level, a
float element as it is) --, with the coordinates, the fractions and the three interpolation steps in float64: the restatement differs from
the kernel by the kernel's own float32 arithmetic and nothing else.  ``warp64`` returns the value of every element BEFORE the output rule
(a stored element or ``fill`` where the rule copies); ``to_output`` (tests/_blur_numpy.py's) applies the output rule.  ``nearest`` is the
exception: it rounds FLOAT32 coordinates (``coords32``) with the float32 ``floor(s + 0.5)``, as the kernel does, so that on rows whose
coordinates are exact in float32 it is the kernel's result element for element."""
from __future__ import annotations

import numpy as np

from tests._blur_numpy import fold, input_values, to_output  # noqa: F401  (the fold and the output rule are blur.hpp's)

MAX_COORD = 4194304.0      # SX_WARP_MAX_COORD = 2^22
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def anchor_row(h: int, w: int, oh: int, ow: int) -> np.ndarray:
    """The row of a tile that is left: (1, 0, (W - OW) div 2, 0, 1, (H - OH) div 2), floor division."""
    return np.array([1.0, 0.0, (w - ow) // 2, 0.0, 1.0, (h - oh) // 2], dtype=np.float32)


def effective_row(row, h: int, w: int, oh: int, ow: int) -> np.ndarray:
    """The float32 row in use: the given one, or the anchor row where one of the six is a NaN or an infinity."""
    row = np.asarray(row, dtype=np.float32).reshape(6)
    return row if np.isfinite(row).all() else anchor_row(h, w, oh, ow)


def coords(row, oh: int, ow: int) -> tuple[np.ndarray, np.ndarray]:
    """(sx, sy), each (OH, OW) float64, of the float32 row: ``a x + b y + c`` and ``d x + e y + f`` evaluated in float64."""
    a, b, c, d, e, f = (float(v) for v in np.asarray(row, dtype=np.float32).reshape(6))
    y, x = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    with np.errstate(over="ignore", invalid="ignore"):
        return a * x + (b * y + c), d * x + (e * y + f)


def _fma32(a, x: np.ndarray, t: np.ndarray) -> np.ndarray:
    """fmaf of float32 operands: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32 (a
    double rounding can differ from the single one in the last place only where the float64 sum is an exact tie of float32: not on the
    rows of these tests, whose coordinates are multiples of 1/16)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=np.float64) * x.astype(np.float64) + t.astype(np.float64)).astype(np.float32)


def coords32(row, oh: int, ow: int) -> tuple[np.ndarray, np.ndarray]:
    """(sx, sy) as the kernel evaluates them: ``fmaf(a, x, fmaf(b, y, c))`` in float32."""
    a, b, c, d, e, f = (np.float32(v) for v in np.asarray(row, dtype=np.float32).reshape(6))
    y, x = np.meshgrid(np.arange(oh, dtype=np.float32), np.arange(ow, dtype=np.float32), indexing="ij")
    return _fma32(a, x, _fma32(b, y, np.full_like(y, c))), _fma32(d, x, _fma32(e, y, np.full_like(y, f)))


def coord_ok(s: np.ndarray) -> np.ndarray:
    """Finite and within the limit (False for a NaN)."""
    with np.errstate(invalid="ignore"):
        return np.abs(s) <= MAX_COORD


def _tap(values: np.ndarray, yi: np.ndarray, xi: np.ndarray, border: str, fill: float) -> np.ndarray:
    """``values[..., yi, xi]`` through the border rule; ``yi``, ``xi``: int64 arrays of one shape."""
    h, w = values.shape[-2:]
    if border == "mirror":
        return values[..., fold(yi, h), fold(xi, w)]
    inside = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
    got = values[..., np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]
    return np.where(inside, got, fill)


def warp64(values: np.ndarray, row, out_size=None, *, interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0) -> np.ndarray:
    """``values``: (..., H, W) float64, every leading axis a plane of its own; ``row``: six numbers, taken as their float32 values.
    -> (..., OH, OW) float64 before the output rule."""
    values = np.asarray(values, dtype=np.float64)
    h, w = values.shape[-2:]
    oh, ow = out_size or (h, w)
    use = effective_row(row, h, w, oh, ow)
    if interpolation == "nearest":
        return nearest(values, use, (oh, ow), border=border, fill=fill)
    sx, sy = coords(use, oh, ow)
    ok = coord_ok(sx) & coord_ok(sy)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        v00, v01 = _tap(values, yi, xi, border, fill), _tap(values, yi, xi + 1, border, fill)
        v10, v11 = _tap(values, yi + 1, xi, border, fill), _tap(values, yi + 1, xi + 1, border, fill)
        top = v00 + fx * (v01 - v00)
        bot = v10 + fx * (v11 - v10)
        out = top + fy * (bot - top)
        out = np.where((fx == 0.0) & (fy == 0.0), v00, out)      # the stored element: no arithmetic touches it (an infinite neighbour times 0 would)
    return np.where(ok, out, fill)


def nearest(values: np.ndarray, row, out_size=None, *, border: str = "mirror", fill: float = 0.0) -> np.ndarray:
    """The stored element at ``(floor(sx + 0.5), floor(sy + 0.5))``, both in float32 on the float32 coordinates, through the border rule."""
    values = np.asarray(values)
    h, w = values.shape[-2:]
    oh, ow = out_size or (h, w)
    sx, sy = coords32(effective_row(row, h, w, oh, ow), oh, ow)
    ok = coord_ok(sx) & coord_ok(sy)
    half = np.float32(0.5)
    xi = np.floor(np.where(ok, sx, np.float32(0)) + half).astype(np.int64)
    yi = np.floor(np.where(ok, sy, np.float32(0)) + half).astype(np.int64)
    return np.where(ok, _tap(values, yi, xi, border, fill), np.asarray(fill, dtype=values.dtype))


def coordinate_slack(row, oh: int, ow: int) -> tuple[float, float]:
    """(Sx, Sy): the sums of the absolute values of a coordinate's three terms at the far corner of the output tile.  A float32
    coordinate is off its exact value by at most 2^-23 S: two roundings, each at most half a unit in the last place of a number <= S."""
    a, b, c, d, e, f = (abs(float(v)) for v in np.asarray(row, dtype=np.float32).reshape(6))
    return a * (ow - 1) + b * (oh - 1) + c, d * (ow - 1) + e * (oh - 1) + f


def rows64(n: int, in_size, out_size=None, *, angle=0.0, scale=1.0, shear=0.0, translate=(0.0, 0.0), flip=False) -> np.ndarray:
    """``affine_rows``' formula in numpy float64, rounded once to float32: (n, 6)."""
    h, w = in_size
    oh, ow = out_size or in_size
    angle, scale, shear, tx, ty = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (angle, scale, shear, translate[0], translate[1]))
    flip = np.broadcast_to(np.asarray(flip, dtype=bool), (n,))
    turn = np.round(angle / 90.0)
    quarter = angle / 90.0 == turn
    k4 = np.mod(turn, 4.0)
    theta = angle * (np.pi / 180.0)
    cos = np.where(quarter, np.where(k4 == 0, 1.0, np.where(k4 == 2, -1.0, 0.0)), np.cos(theta))
    sin = np.where(quarter, np.where(k4 == 1, 1.0, np.where(k4 == 3, -1.0, 0.0)), np.sin(theta))
    k = np.tan(shear * (np.pi / 180.0))
    m = np.where(flip, -1.0, 1.0)
    a, b, d, e = m * (cos - k * sin) / scale, m * (-sin - k * cos) / scale, sin / scale, cos / scale
    ux, uy = (ow - 1) / 2.0 + tx, (oh - 1) / 2.0 + ty
    c = (w - 1) / 2.0 - a * ux - b * uy
    f = (h - 1) / 2.0 - d * ux - e * uy
    return np.stack([a, b, c, d, e, f], axis=1).astype(np.float32)


def scipy_arguments(row) -> tuple[np.ndarray, np.ndarray]:
    """(matrix, offset) of ``scipy.ndimage.affine_transform`` for a row: scipy's coordinates are (row, column)."""
    a, b, c, d, e, f = (float(v) for v in np.asarray(row, dtype=np.float32).reshape(6))
    return np.array([[e, d], [b, a]]), np.array([f, c])
