"""The JPEG round trip of include/stainx_hip.h (sx_jpeg_roundtrip) in numpy int64, vectorised over 8 x 8 blocks: the definition the GPU
tests compare against.  Every step is the header's: JFIF colour through libjpeg's 16-bit tables, 4:2:0 chroma down (2 x 2 mean with the
alternating bias), the "islow" forward DCT, quantisation by integer division, dequantisation, the "islow" inverse DCT, the triangle
chroma filter (plain replication where the chroma plane is at most two columns wide) and the colour conversion back.  Nothing here is
tuned to the kernel: it agrees byte for byte with Pillow / libjpeg-turbo (tests/test_jpeg_cpu.py, tests/golden/jpeg_pillow.npz).
"""
from __future__ import annotations

import numpy as np

LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMINANCE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64).reshape(8, 8)
SUBSAMPLING = {"444": 0, "420": 2, 0: 0, 2: 2}


def D(x, n):
    return (x + (1 << (n - 1))) >> n


def tables(quality: float) -> tuple[np.ndarray, np.ndarray]:
    """The (8, 8) luminance and chrominance tables of a quality >= 1 (above 100 is 100)."""
    q = min(int(quality), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMINANCE, CHROMINANCE))


def levels_of(x: np.ndarray) -> np.ndarray:
    """The 8-bit levels a tile stands for: a uint8 byte is its level; a float element is taken to float32, multiplied by 255 in float32 and
    rounded to the nearest even integer, clamped to 0..255; a NaN is level 0."""
    if x.dtype == np.uint8:
        return x.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(x.astype(np.float32) * np.float32(255.0))
    return np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 255.0).astype(np.int64)


def _odd(t4, t5, t6, t7):
    """The odd part both transforms share: the four sums that go to outputs 7, 5, 3, 1 (forward) or are combined with the even part (inverse)."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _forward_pass(d, row_pass: bool):
    """One pass of jfdctint over the LAST axis (length 8)."""
    d = [d[..., i] for i in range(8)]
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if row_pass else 15
    out = [None] * 8
    out[0] = (t10 + t11) * 4 if row_pass else D(t10 + t11, 2)
    out[4] = (t10 - t11) * 4 if row_pass else D(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = D(z1 + t13 * 6270, n)
    out[6] = D(z1 - t12 * 15137, n)
    o7, o5, o3, o1 = _odd(t4, t5, t6, t7)
    out[7], out[5], out[3], out[1] = D(o7, n), D(o5, n), D(o3, n), D(o1, n)
    return np.stack(out, axis=-1)


def _inverse_pass(c, n: int):
    """One pass of jidctint over the LAST axis."""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) * 8192, (c[0] - c[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = _odd(c[7], c[5], c[3], c[1])
    out = [D(t10 + o3, n), D(t11 + o2, n), D(t12 + o1, n), D(t13 + o0, n), D(t13 - o0, n), D(t12 - o1, n), D(t11 - o2, n), D(t10 - o3, n)]
    return np.stack(out, axis=-1)


def forward_dct(blocks: np.ndarray) -> np.ndarray:
    """(..., 8, 8) levels minus 128 -> coefficients with a factor of 8: rows, then columns."""
    rows = _forward_pass(blocks, True)
    return np.swapaxes(_forward_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def inverse_dct(coefficients: np.ndarray) -> np.ndarray:
    """(..., 8, 8) dequantised coefficients -> levels 0..255: columns, then rows, + 128, clamped."""
    columns = np.swapaxes(_inverse_pass(np.swapaxes(coefficients, -1, -2), 11), -1, -2)
    return np.clip(_inverse_pass(columns, 18) + 128, 0, 255)


def quantise(coefficients: np.ndarray, table: np.ndarray) -> np.ndarray:
    return np.sign(coefficients) * ((np.abs(coefficients) + ((8 * table) >> 1)) // (8 * table))


def code_plane(plane: np.ndarray, table: np.ndarray) -> np.ndarray:
    """A plane whose sides are multiples of 8 through forward DCT, quantiser, dequantiser and inverse DCT."""
    h, w = plane.shape
    blocks = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128
    decoded = inverse_dct(quantise(forward_dct(blocks), table) * table)
    return decoded.transpose(0, 2, 1, 3).reshape(h, w)


def _extend(plane: np.ndarray, rows: int, columns: int) -> np.ndarray:
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, columns - plane.shape[1])), mode="edge")


def _up(n: int, to: int) -> int:
    return -(-n // to) * to


def chroma_down(plane: np.ndarray) -> np.ndarray:
    """4:2:0: right edge replicated to a multiple of 16 columns, bottom row to an even height, the 2 x 2 mean with bias 1 / 2 in even /
    odd output columns, then the last DOWNSAMPLED row replicated to a multiple of 8 rows."""
    h, w = plane.shape
    p = _extend(plane, h + (h & 1), _up(w, 16))
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    d = (s + 1 + (np.arange(s.shape[1]) & 1)) >> 2
    return _extend(d, _up(d.shape[0], 8), d.shape[1])


def chroma_up(plane: np.ndarray, h: int, w: int) -> np.ndarray:
    """The decoded chroma plane cropped to ceil(h / 2) x ceil(w / 2) -> h x w: the triangle filter, edges replicated; plain 2 x 2
    replication where the cropped plane is at most two columns wide."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    c = plane[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    t = np.empty((2 * ch, cw), dtype=np.int64)
    t[0::2], t[1::2] = 3 * c + above, 3 * c + below
    left, right = np.concatenate([t[:, :1], t[:, :-1]], axis=1), np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * t + left + 8) >> 4, (3 * t + right + 7) >> 4
    return out[:h, :w]


def roundtrip_levels(levels: np.ndarray, quality: float, subsampling) -> np.ndarray:
    """(3, H, W) levels 0..255 -> (3, H, W) uint8: what a baseline JPEG of that quality and subsampling decodes to."""
    sub = SUBSAMPLING[subsampling]
    r, g, b = (levels[i].astype(np.int64) for i in range(3))
    h, w = r.shape
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    luma, chroma = tables(quality)
    y = code_plane(_extend(y, _up(h, 8), _up(w, 8)), luma)[:h, :w]
    if sub == 0:
        cb, cr = (code_plane(_extend(c, _up(h, 8), _up(w, 8)), chroma)[:h, :w] for c in (cb, cr))
    else:
        cb, cr = (chroma_up(code_plane(chroma_down(c), chroma), h, w) for c in (cb, cr))
    cb, cr = cb - 128, cr - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)])
    return np.clip(out, 0, 255).astype(np.uint8)


def roundtrip(tiles: np.ndarray, qualities, subsampling="420") -> np.ndarray:
    """(N, 3, H, W) uint8 or float tiles and one quality per tile (or one for all) -> (N, 3, H, W) uint8 levels; a tile whose quality is
    NaN, infinite or below 1 keeps its own levels."""
    qualities = np.broadcast_to(np.asarray(qualities, dtype=np.float32).reshape(-1), (tiles.shape[0],))
    out = np.empty(tiles.shape, dtype=np.uint8)
    for i, q in enumerate(qualities):
        lv = levels_of(tiles[i])
        out[i] = roundtrip_levels(lv, float(q), subsampling) if np.isfinite(q) and q >= 1 else lv.astype(np.uint8)
    return out
