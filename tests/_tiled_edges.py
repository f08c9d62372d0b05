"""Shapes and parameter rows for the kernels that cut a tile into fixed blocks held in LDS -- blur (blur.hpp), the JPEG round trip
(jpeg.hpp), focus (focus.hpp), the affine and the elastic warp (warp.hpp, elastic.hpp) -- chosen for the case their own test files hardly
reach: a block ON THE PACK PATH that the tile's edge cuts.  numpy and torch on the CPU only; tests/test_tiled_edges_cpu.py holds what is
here to the kernels' constants and to the restatements, tests/test_tiled_edges_gpu.py runs it on the device.

THE SHAPE RULE.  Each of these kernels moves 4-pixel packs where ``W % 4 == 0`` (and the pointers allow it) and single elements
otherwise.  A shape (H, W) is RAGGED ON THE PACK PATH for a kernel whose block is B columns wide when ``W % 4 == 0 and W % B != 0``; for a
tile narrower than a block that is ``W < B``.  Then the last block of a row holds ``W % B`` columns: packs up to the tile's edge, and
behind it whatever the kernel does with a pack that lies outside the row (blur: reflected single elements; focus: the reflected column
``W``; JPEG: the replicated last column of the 8-column block extension; the copy paths: nothing).  ``classify`` states the rule once;
``SHAPES`` lists, per kernel, the shapes with the classification the CPU test asserts -- a later change of a block size shows up there as
a failing assertion, not as coverage that is silently lost.

The block sizes, as the sources state them (the CPU test reads them back from the sources):
    blur     kBlurSide = 64                                            (blur.hpp)
    jpeg     kJpegRegionW = 128, kJpegRegionH444 = 64, kJpegRegionH420 = 128; blocks of 8, MCUs of 16 in 4:2:0   (jpeg_block.hpp)
    focus    kFocusRows = 64, kFocusCols = 64                          (focus.hpp)
    warp     kWarpSide = 32 (elastic.hpp uses the same constant)       (warp.hpp)
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

from tests import _blur_numpy as bn
from tests import _focus_numpy as fn

F32 = np.float32
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)

# ------------------------------------------------------------------ 1. the shape rule
BLOCKS = {"blur": (64, 64), "jpeg444": (64, 128), "jpeg420": (128, 128), "focus": (64, 64), "warp": (32, 32)}      # (rows, columns) of a workgroup's block
CONSTANTS = {      # source file -> the constants BLOCKS restates
    "blur.hpp": {"kBlurSide": 64, "kBlurMaxRadius": 16},
    "jpeg_block.hpp": {"kJpegRegionW": 128, "kJpegRegionH444": 64, "kJpegRegionH420": 128},
    "focus.hpp": {"kFocusRows": 64, "kFocusCols": 64},
    "warp.hpp": {"kWarpSide": 32},
}


def classify(h: int, w: int, block: tuple) -> dict:
    """What a kernel with a ``block`` = (rows, columns) makes of an (H, W) tile."""
    bh, bw = block
    across, down = -(-w // bw), -(-h // bh)
    pack = w % 4 == 0
    return {"pack": pack, "across": across, "down": down, "last_cols": w - (across - 1) * bw, "last_rows": h - (down - 1) * bh, "ragged": pack and w % bw != 0}


# shape -> (blocks across, blocks down, columns in the last block, rows in the last block); every one is ragged on the pack path
BLUR_SHAPES = {(1, 4): (1, 1, 4, 1), (3, 12): (1, 1, 12, 3), (9, 36): (1, 1, 36, 9), (5, 68): (2, 1, 4, 5), (66, 100): (2, 2, 36, 2), (8, 132): (3, 1, 4, 8), (130, 68): (2, 3, 4, 2)}
FOCUS_SHAPES = {(2, 3, 8): (1, 1, 8, 3), (2, 5, 60): (1, 1, 60, 5), (3, 9, 68): (2, 1, 4, 9), (2, 70, 132): (3, 2, 4, 6)}      # (N, H, W)
WARP_SHAPES = {(5, 36): (2, 1, 4, 5), (33, 40): (2, 2, 8, 1), (40, 100): (4, 2, 4, 8)}
# JPEG: shape -> (W % 8, regions across, regions down in 4:4:4, regions down in 4:2:0, columns in the last region)
JPEG_SHAPES = {(8, 4): (4, 1, 1, 1, 4), (5, 12): (4, 1, 1, 1, 12), (16, 20): (4, 1, 1, 1, 20), (9, 136): (0, 2, 1, 1, 8), (24, 132): (4, 2, 1, 1, 4), (16, 264): (0, 3, 1, 1, 8),
               (136, 12): (4, 1, 3, 2, 12), (72, 132): (4, 2, 2, 1, 4), (136, 132): (4, 2, 3, 2, 4)}
SHAPES = {"blur": BLUR_SHAPES, "focus": FOCUS_SHAPES, "warp": WARP_SHAPES, "jpeg": JPEG_SHAPES}
MAX_PIXELS = 20000


def ids(shapes) -> list:
    return ["x".join(str(v) for v in s) for s in shapes]


# ------------------------------------------------------------------ 2. blur: the sigma rows
RAGGED_SIGMAS = (0.3, 1.7, 4.0, NAN, 7.0)      # radii 1, 7 and 16, a copy tile, a clamped sigma (R = 16): one launch
RAGGED_RADII = (1, 7, 16, 0, 16)


def below(x) -> np.float32:
    return np.nextafter(F32(x), F32(-np.inf))


def above(x) -> np.float32:
    return np.nextafter(F32(x), F32(np.inf))


def border_sigmas() -> tuple:
    """The 16 borders of R = (int)(4 sigma + 0.5): (k + 0.5) / 4 for k = 0..15, each exact in float32; R is k below it and k + 1 from it on."""
    return tuple(float(F32((k + 0.5) / 4.0)) for k in range(16))


@lru_cache(maxsize=None)
def radius_sigmas() -> tuple:
    """Every border with its two float32 neighbours, R / 4 for R = 1..16 (the middle of radius R's interval), 4.0 (again: the clamp's own
    value, on another tile) and the float above it: 66 sigmas, Python floats of float32 values."""
    out = []
    for s in border_sigmas():
        out += [float(below(s)), s, float(above(s))]
    out += [r / 4.0 for r in range(1, 17)]
    out += [4.0, float(above(4.0))]
    assert all(float(F32(s)) == s for s in out)
    return tuple(out)


@lru_cache(maxsize=None)
def impulse_sigmas() -> tuple:
    """One sigma per radius 1..16 (R / 4) and, for every border, the border itself and the float below it: the two sides of each step."""
    out = [r / 4.0 for r in range(1, 17)]
    for s in border_sigmas():
        out += [float(below(s)), s]
    return tuple(out)


def taps32(sigma) -> np.ndarray:
    """The R + 1 taps w_0..w_R as blur.hpp evaluates them, in numpy float32: scale = -0.5f / (sigma * sigma), w_i = expf((float)(i * i) *
    scale), the sum w_0 + 2 w_1 + ... taken in order, each tap divided by it.  (numpy's float32 exp stands for expf.)"""
    s = min(F32(sigma), F32(bn.MAX_SIGMA))
    r = bn.radius(sigma)
    scale = F32(-0.5) / (s * s)
    w = [np.exp(F32(i * i) * scale, dtype=F32) for i in range(r + 1)]
    total = F32(0.0)
    for i, v in enumerate(w):
        total = total + (v if i == 0 else F32(2.0) * v)
    return np.array([v / total for v in w], dtype=F32)


REL = 2.0**-15      # the impulse response's relative bound: see tests/test_tiled_edges_gpu.py's docstring


# ------------------------------------------------------------------ tiles
@lru_cache(maxsize=None)
def blur_tiles(dtype: torch.dtype, shape: tuple, n: int) -> torch.Tensor:
    """(n, 3, H, W) on the CPU, tests/test_blur_gpu.py's recipe for any number of tiles: seeded uint8 levels, or seeded float32 uniforms in
    [0, 1) rounded to the type."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + 7 * n)
    if dtype == torch.uint8:
        return torch.from_numpy(rng.integers(0, 256, size=(n, 3, *shape), dtype=np.uint8))
    return torch.from_numpy(rng.random((n, 3, *shape), dtype=np.float32)).to(dtype)


@lru_cache(maxsize=None)
def blur_reference(dtype: torch.dtype, shape: tuple, sigmas: tuple) -> np.ndarray:
    """(n, 3, H, W) float64: tile t of ``blur_tiles(dtype, shape, len(sigmas))`` under sigma t, before the output rule.  Computed once."""
    x = blur_tiles(dtype, shape, len(sigmas))
    out = np.stack([bn.blur64(bn.input_values(x[t]), s) for t, s in enumerate(sigmas)])
    out.setflags(write=False)
    return out


IMPULSE_SHAPES = ((100, 132), (9, 36))


def impulse_places(shape: tuple) -> tuple:
    """Two tiles' worth of (row, column) per channel.  100 x 132: the middle of a block (32 from its seams and the border), a block corner
    (row 63 / column 64: the last row of one block, the first column of the next), the ragged last block three columns from the right edge;
    then the two corner pixels of the tile and the ragged block's last row.  9 x 36 (one ragged block, every axis shorter than the largest
    halo): the centre, three columns from the right edge, a corner; the other corners."""
    h, w = shape
    if shape == (100, 132):
        return (((32, 32), (63, 64), (40, w - 3)), ((0, 0), (h - 1, w - 1), (h - 1, w - 4)))
    return (((h // 2, w // 2), (2, w - 3), (0, 0)), ((h - 1, w - 1), (0, w - 1), (h - 1, 0)))


@lru_cache(maxsize=None)
def impulse_tiles(shape: tuple) -> tuple:
    """((T, 3, H, W) float32 tiles of +0.0 with a single 1.0 per channel, the T sigmas, the T place triples): every sigma of
    ``impulse_sigmas`` with both place triples of the shape."""
    places, sigmas, where = impulse_places(shape), [], []
    for s in impulse_sigmas():
        for triple in places:
            sigmas.append(s)
            where.append(triple)
    x = torch.zeros((len(sigmas), 3, *shape), dtype=torch.float32)
    for t, triple in enumerate(where):
        for c, (y, col) in enumerate(triple):
            x[t, c, y, col] = 1.0
    return x, tuple(sigmas), tuple(where)


@lru_cache(maxsize=None)
def impulse_reference(shape: tuple) -> np.ndarray:
    x, sigmas, _ = impulse_tiles(shape)
    out = np.stack([bn.blur64(x[t].numpy().astype(np.float64), s) for t, s in enumerate(sigmas)])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ 3. JPEG
JPEG_QUALITIES = (10.0, 50.0, 95.0, NAN)
QUALITY_SHAPE = (16, 24)      # 4:2:0: one and a half MCUs wide
# the quality rule: finite rows at or above 1 code with min((int)q, 100); the rest leave their tile
RULE_ROWS = (1.0, 1.999, 49.999, 50.0, 50.5, 99.999, 100.0, 150.0, 1e30, 3.0e38, 3.2e38, FLT_MAX, 0.999, 0.0, -5.0, -0.0, INF, -INF, NAN)
RULE_QUALITY = (1, 1, 49, 50, 50, 99, 100, 100, 100, 100, 100, 100, 0, 0, 0, 0, 0, 0, 0)      # 0: a copy
RULE_SHAPE = (16, 20)


@lru_cache(maxsize=None)
def jpeg_tiles(shape: tuple, n: int) -> np.ndarray:
    """(n, 3, H, W) uint8, read-only: even tiles seeded bytes (large coefficients: the reciprocal divide's whole range), odd tiles crops of
    the real-tissue fixture (small coefficients, next to the quantiser's ties)."""
    h, w = shape
    rng = np.random.default_rng(100 * h + w + n)
    out = rng.integers(0, 256, size=(n, 3, h, w), dtype=np.uint8)
    real = fn.real_crop()      # (3, 3, 150, 203)
    per_row, per_tile = real.shape[3] // w, (real.shape[2] // h) * (real.shape[3] // w)
    assert per_tile * real.shape[0] >= n // 2
    for t in range(1, n, 2):
        k = t // 2
        i, j = divmod(k % per_tile, per_row)
        out[t] = real[k // per_tile, :, i * h:(i + 1) * h, j * w:(j + 1) * w]
    out.setflags(write=False)
    return out


def every_quality() -> tuple:
    return tuple(float(q) for q in range(1, 101))


# ------------------------------------------------------------------ 5. the warps' copy path
LEFT_ROWS = ((NAN,) * 6, (1.0, 0.0, INF, 0.0, 1.0, 0.0), (0.96875, -0.125, 1.25, 0.125, 0.96875, -0.75))      # a NaN row, an infinite row, a finite row: a mixed launch
SPECIAL_BITS = (0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000)      # NaN payloads, -0.0, infinities, a denormal, 1.0


def with_specials(x: torch.Tensor) -> torch.Tensor:
    """A float tile batch with every fifth element one of SPECIAL_BITS' float32 values converted to the type (float64: no NaN, whose
    payload a conversion to float32 and back need not keep)."""
    patterns = torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    if x.dtype == torch.float64:
        patterns = patterns[2:]
    flat = x.clone().reshape(-1)
    count = flat[::5].numel()
    flat[::5] = patterns.repeat(count // patterns.numel() + 1)[:count].to(x.dtype)
    return flat.reshape(x.shape)
