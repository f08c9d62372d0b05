"""The yardstick of the mask components, written without the library and without scipy: a plain two-pass union-find over the set pixels
(tests/test_components_cpu.py pins it to a canonicalised scipy.ndimage.label), areas and counts by bincount, the area filters in one
line each, and the mask generators both test files share.

Label of a set pixel: 1 + (y * W + x) of the first pixel of its component in raster order within its tile; 0 of an unset pixel."""
from __future__ import annotations

import functools

import numpy as np

CONNECTIVITIES = (4, 8)
DENSITIES = (0.3, 0.41, 0.5, 0.593, 0.8)      # around the site-percolation thresholds of the two connectivities (0.407 under 8, 0.593 under 4)


# ------------------------------------------------------------------ labelling
def label_tile(mask: np.ndarray, connectivity: int) -> np.ndarray:
    """(H, W) int32 canonical labels of one tile.  First pass: every set pixel, in raster order, is united with its set neighbours that
    came before it (left and up; the two upper diagonals too under 8), the smaller root staying the root -- so a root is the first
    pixel of its component.  Second pass: every set pixel takes its root."""
    assert connectivity in CONNECTIVITIES
    h, w = mask.shape
    stride = w + 2
    padded = np.zeros((h + 1, stride), dtype=bool)      # a clear row above, a clear column left and right: no bounds checks below
    padded[1:, 1:-1] = mask != 0
    is_set = padded.ravel().tolist()
    pixels = np.flatnonzero(padded.ravel())
    parent = list(range(len(is_set)))
    before = (-1, -stride) if connectivity == 4 else (-1, -stride - 1, -stride, -stride + 1)

    def find(i: int) -> int:
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    for i in pixels.tolist():
        for off in before:
            if is_set[i + off]:
                a, b = find(i), find(i + off)
                if a < b:
                    parent[b] = a
                elif b < a:
                    parent[a] = b
    roots = np.array([find(i) for i in pixels.tolist()], dtype=np.int64)
    labels = np.zeros(h * w, dtype=np.int32)
    own = (pixels // stride - 1) * w + pixels % stride - 1
    labels[own] = (roots // stride - 1) * w + roots % stride - 1 + 1
    return labels.reshape(h, w)


def components(mask: np.ndarray, connectivity: int = 8, holes: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(labels, areas, counts) of a batch (N, H, W): int32, int32, int64 -- what stainx_amd.mask_components returns."""
    bits = (mask != 0) != bool(holes)
    n, h, w = bits.shape
    labels = np.stack([label_tile(tile, connectivity) for tile in bits]) if n else np.zeros((0, h, w), dtype=np.int32)
    sizes = np.stack([np.bincount(tile.ravel(), minlength=h * w + 1) for tile in labels])
    sizes[:, 0] = 0
    areas = sizes[:, 1:].reshape(n, h, w).astype(np.int32)
    return labels, areas, (areas != 0).sum(axis=(1, 2)).astype(np.int64)


def pixel_areas(labels: np.ndarray, areas: np.ndarray) -> np.ndarray:
    """The area of every pixel's component (0 for an unset pixel)."""
    n = labels.shape[0]
    flat = np.concatenate([np.zeros((n, 1), dtype=areas.dtype), areas.reshape(n, -1)], axis=1)
    return np.take_along_axis(flat, labels.reshape(n, -1).astype(np.int64), axis=1).reshape(labels.shape)


def objects_kept(labels: np.ndarray, areas: np.ndarray, min_area: int) -> np.ndarray:
    """remove_small_objects from the components of the mask: an unset pixel has area 0 < 1 <= min_area."""
    return (pixel_areas(labels, areas) >= min_area).astype(np.uint8)


def holes_filled(labels: np.ndarray, areas: np.ndarray, min_area: int) -> np.ndarray:
    """remove_small_holes from the components of the COMPLEMENT: a set pixel has area 0 there and stays set."""
    return (pixel_areas(labels, areas) < min_area).astype(np.uint8)


def remove_small_objects(mask: np.ndarray, min_area: int, connectivity: int = 8) -> np.ndarray:
    return objects_kept(*components(mask, connectivity)[:2], min_area)


def remove_small_holes(mask: np.ndarray, min_area: int, connectivity: int = 8) -> np.ndarray:
    return holes_filled(*components(mask, connectivity, holes=True)[:2], min_area)


def canonical(labelled: np.ndarray) -> np.ndarray:
    """Arbitrary positive labels of one tile (scipy.ndimage.label's) -> the canonical ones."""
    flat = labelled.ravel()
    first = np.full(int(flat.max()) + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return np.where(flat > 0, first[flat] + 1, 0).astype(np.int32).reshape(labelled.shape)


# ------------------------------------------------------------------ mask generators: (H, W) uint8, 1 / 0
def serpentine(h: int, w: int) -> np.ndarray:
    """Every second row set, joined alternately at the right and the left end: one component, a path about H * W / 2 long."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def checkerboard(h: int, w: int) -> np.ndarray:
    """H * W / 2 components of area 1 under 4, one component under 8."""
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0).astype(np.uint8)


def comb(h: int, w: int) -> np.ndarray:
    """Vertical teeth on every second column joined only by a bar along the last row."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[:, 0::2] = 1
    m[h - 1] = 1
    return m


def diagonal(h: int, w: int) -> np.ndarray:
    """A one-pixel main diagonal and a one-pixel anti-diagonal, placed (where the tile is large enough) to pass exactly through the
    corner at row 256, column 64 of a 256 x 64 block grid: (255, 63) - (256, 64) and (255, 64) - (256, 63)."""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    big = h > 256 and w > 64
    return ((y - x == (192 if big else 0)) | (y + x == (319 if big else w - 1))).astype(np.uint8)


def random(h: int, w: int, density: float, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def frames(h: int, w: int) -> np.ndarray:
    """Nested one-pixel rectangles two apart: holes inside holes."""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return (np.minimum(np.minimum(y, h - 1 - y), np.minimum(x, w - 1 - x)) % 2 == 0).astype(np.uint8)


GENERATORS = ("serpentine", "checkerboard", "comb", "diagonal", "frames") + tuple(f"random_{d}" for d in DENSITIES)


def tile(name: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    if name.startswith("random_"):
        return random(h, w, float(name.split("_")[1]), 1000 + seed)
    return {"serpentine": serpentine, "checkerboard": checkerboard, "comb": comb, "diagonal": diagonal, "frames": frames}[name](h, w)


# The batches of the GPU tests: every generator once per shape, dealt into batches of the shape's N tiles (the last batch filled up
# with further random tiles).  Computed once per process and never written to.
@functools.lru_cache(maxsize=None)
def batches(n: int, h: int, w: int) -> tuple[tuple[tuple[str, ...], np.ndarray], ...]:
    names = list(GENERATORS)
    while len(names) % n:
        names.append(f"random_{DENSITIES[len(names) % len(DENSITIES)]}")
    out = []
    for at in range(0, len(names), n):
        group = tuple(names[at:at + n])
        mask = np.stack([tile(name, h, w, seed=at + i) for i, name in enumerate(group)])
        mask.setflags(write=False)
        out.append((group, mask))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def batch_components(n: int, h: int, w: int, index: int, connectivity: int, holes: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    result = components(batches(n, h, w)[index][1], connectivity, holes)
    for part in result:
        part.setflags(write=False)
    return result
