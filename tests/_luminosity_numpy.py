"""float64 restatement of luminosity standardisation (stainx_amd.LuminosityStandardizer, include/stainx_hip.h: sx_luminosity_*): the
rank rule in Python doubles, and the map for a GIVEN luminance percentile Y_p.  The reference of the tolerance checks; the percentile
itself is checked exactly, against sx_tissue_mask_tiles, and needs no restatement."""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=np.float64)
XYZ2RGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]], dtype=np.float64)
WHITE = np.array([0.95047, 1.0, 1.08883], dtype=np.float64).reshape(1, 3, 1, 1)


def real_images() -> np.ndarray:
    """(6, 3, 1024, 1024) uint8: the six real H&E images of the golden set."""
    with np.load(GOLDEN / "g11_real_images.npz", allow_pickle=False) as z:
        return z["images_u8"]


def rank(count: int, percentile: float) -> int:
    """k = 1 + rint((0.01 * percentile) * (double)(count - 1)), half to even, in doubles; 0 for an empty set."""
    if count <= 0:
        return 0
    return 1 + int(round((0.01 * float(percentile)) * float(count - 1)))      # (round() of a float: half to even)


def unit(images: np.ndarray) -> np.ndarray:
    """The unit values in float64: uint8 / 255, floats as they are (a half-precision input: its rounded value)."""
    x = np.asarray(images)
    return x.astype(np.float64) / 255.0 if x.dtype == np.uint8 else x.astype(np.float64)


def linear(u: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where(u > 0.04045, np.power((u + 0.055) / 1.055, 2.4), u / 12.92)


def f_of(t: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def f_inv(t: np.ndarray) -> np.ndarray:
    return np.where(t > 0.2068966, t ** 3, (t - 16.0 / 116.0) / 7.787)


def luminance(images: np.ndarray) -> np.ndarray:
    """Y (N, H, W) in float64: the colour conversion's middle row on the linear-light values."""
    lin = linear(unit(images))
    return RGB2XYZ[1, 0] * lin[:, 0] + RGB2XYZ[1, 1] * lin[:, 1] + RGB2XYZ[1, 2] * lin[:, 2]


def lightness(y: np.ndarray | float) -> np.ndarray:
    """L* in 0..100 of a luminance."""
    return 116.0 * f_of(np.asarray(y, dtype=np.float64)) - 16.0


def gain(y_p: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(g, through) per row: g = 100 / L_p; through where Y_p is NaN, L_p <= 0 or Y_p is exactly 1 (gain 1) (the tile is copied)."""
    y_p = np.asarray(y_p, dtype=np.float64).reshape(-1)
    l_p = lightness(y_p)
    through = np.isnan(y_p) | ~(l_p > 0.0) | (y_p == 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(through, 1.0, 100.0 / l_p), through


def f_values(images: np.ndarray) -> np.ndarray:
    """(f_x, f_y, f_z) (N, 3, H, W) of the LAB conversion."""
    xyz = np.einsum("ij,njhw->nihw", RGB2XYZ, linear(unit(images))) / WHITE
    return f_of(xyz)


def from_f(f: np.ndarray) -> np.ndarray:
    """(f_x, f_y, f_z) back to unit sRGB, clamped."""
    lin = np.einsum("ij,njhw->nihw", XYZ2RGB, f_inv(f) * WHITE)
    with np.errstate(invalid="ignore"):
        rgb = np.where(lin > 0.0031308, 1.055 * np.power(lin, 1.0 / 2.4) - 0.055, 12.92 * lin)
    return np.clip(rgb, 0.0, 1.0)


def standardize_unit(images: np.ndarray, y_p: np.ndarray) -> np.ndarray:
    """The map in float64, unit values out: f_y' = min(g f_y + (16/116)(1 - g), 1), f_x' = f_y' + (f_x - f_y), f_z' = f_y' - (f_y - f_z).
    ``y_p``: one luminance, or one per tile.  Tiles that are copied through keep their unit values."""
    images = np.asarray(images)
    n = images.shape[0]
    g, through = gain(y_p)
    if g.shape[0] == 1:
        g, through = np.repeat(g, n), np.repeat(through, n)
    g = g.reshape(n, 1, 1)
    f = f_values(images)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    fy2 = np.minimum(g * fy + (16.0 / 116.0) * (1.0 - g), 1.0)
    out = from_f(np.stack([fy2 + (fx - fy), fy2, fy2 - (fy - fz)], axis=1))
    out[through] = unit(images)[through]
    return out


def to_levels(out_unit: np.ndarray) -> np.ndarray:
    """uint8 as the library stores it: clamp(255 x, 0, 255), truncated."""
    return np.trunc(np.clip(out_unit * 255.0, 0.0, 255.0)).astype(np.uint8)


def lab_round_trip(images: np.ndarray, y_p: float, rgb_to_lab, lab_to_rgb) -> np.ndarray:
    """The same map step by step through GIVEN conversions (the oracle's: scaled LAB, L* 2.55, a + 128, b + 128): only L* is changed,
    L*' = min(100 L* / L_p, 100)."""
    lab = rgb_to_lab(unit(images).astype(np.float32)).astype(np.float64)
    l_star = lab[:, 0] / 2.55
    lab[:, 0] = np.minimum(100.0 * l_star / float(lightness(y_p)), 100.0) * 2.55
    return lab_to_rgb(lab.astype(np.float32)).astype(np.float64)
