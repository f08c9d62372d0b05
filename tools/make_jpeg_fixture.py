"""Writes tests/golden/jpeg_pillow.npz: seeded uint8 tiles and what Pillow (libjpeg) returns for them after one JPEG round trip, the bytes
that pin tests/_jpeg_numpy.py -- and through it sx_jpeg_roundtrip -- where Pillow is not installed.  Needs Pillow; run from the repository
root:  python tools/make_jpeg_fixture.py

Keys: ``in_HxW`` (3, H, W) uint8 and ``out_HxW_qQ_sS`` (3, H, W) uint8 for the shapes, qualities 1 / 35 / 75 / 100 and subsamplings 0
(4:4:4) and 2 (4:2:0) below; ``in_real`` -- rows and columns 448..575 of the first image of g11_real_images.npz -- with ``out_real_q50_sS``
and ``out_real_q90_sS``; ``pillow`` the version string.
"""
from __future__ import annotations

import io
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (8, 8), (9, 17), (16, 16), (17, 9), (33, 31), (65, 130))
QUALITIES = (1, 35, 75, 100)
REAL_CROP = (slice(448, 576), slice(448, 576))


def pillow_roundtrip(chw: np.ndarray, quality: int, subsampling: int) -> np.ndarray:
    buffer = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)), "RGB").save(buffer, "JPEG", quality=int(quality), subsampling=int(subsampling))
    buffer.seek(0)
    return np.ascontiguousarray(np.asarray(Image.open(buffer).convert("RGB")).transpose(2, 0, 1))


def seeded_tile(h: int, w: int) -> np.ndarray:
    """A smooth colour ramp plus noise (so that every quality keeps some coefficients and drops others), seeded by the shape."""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([40 + 3 * yy + 2 * xx, 200 - 2 * yy + xx, 90 + yy - 3 * xx]).astype(np.float64)
    return np.clip(base + rng.normal(0.0, 25.0, (3, h, w)), 0, 255).astype(np.uint8)


def main() -> None:
    arrays = {"pillow": np.array(PIL.__version__)}
    for h, w in SHAPES:
        tile = seeded_tile(h, w)
        arrays[f"in_{h}x{w}"] = tile
        for q in QUALITIES:
            for s in (0, 2):
                arrays[f"out_{h}x{w}_q{q}_s{s}"] = pillow_roundtrip(tile, q, s)
    real = np.load(ROOT / "tests" / "golden" / "g11_real_images.npz")["images_u8"][0][(slice(None),) + REAL_CROP]
    arrays["in_real"] = np.ascontiguousarray(real)
    for q in (50, 90):
        for s in (0, 2):
            arrays[f"out_real_q{q}_s{s}"] = pillow_roundtrip(real, q, s)
    path = ROOT / "tests" / "golden" / "jpeg_pillow.npz"
    np.savez_compressed(path, **arrays)
    print(f"{path}: {path.stat().st_size} bytes, {len(arrays)} arrays, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
