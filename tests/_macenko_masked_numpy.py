"""The yardstick of the masked-Macenko tests: the reference's algorithm restated on the masked-in pixels only, from the CPU oracle's own
functions (oracle/stain_oracle.py, imported and unchanged).  Estimate: ``so.macenko_tile_params`` of exactly the masked-in optical
densities; transform: the tail of ``so.macenko_transform`` on those pixels; background: the input's level on the 0-255 scale through the
same clamp and cast.  With an all-ones mask every function returns exactly what the oracle's unmasked one returns
(tests/test_macenko_mask_cpu.py pins that).  Also the mask builders both test files use."""
from __future__ import annotations

import numpy as np

from oracle import stain_oracle as so

F32 = np.float32


# ------------------------------------------------------------------ the estimate
PLANE_FLOOR = 1e-6      # (see plane_defined)


def plane_defined(od_3xk: np.ndarray) -> bool:
    """Whether the pixel set the fit runs on spans a plane at all: the middle eigenvalue of its covariance (float64) against the mean
    square of the optical densities.  The densities are float32 values of order 1, so the covariance the reference forms from them carries
    rounding of about 2^-24 ~ 6e-8 of that mean square per entry; a middle eigenvalue under ``PLANE_FLOOR`` (1e-6, an order above that
    noise) is not told from zero, and the eigenvectors of a zero matrix -- the stain plane, HE and maxC after it -- are whatever the
    eigen-solver's rounding makes them, in the reference as anywhere else.  A constant tile (``synth.he_batch`` below 16 x 16 is one: its
    concentration map has a single cell) gives exactly 0 here; every textured tile the tests use gives 1e-3 or more."""
    if od_3xk.shape[1] < 3:
        return False
    od = od_3xk.astype(np.float64)
    return bool(np.linalg.eigvalsh(np.cov(od))[1] > PLANE_FLOOR * np.mean(od * od))


def group_estimate(od_3xp: np.ndarray, mask_p: np.ndarray, *, per_tile: bool, signs=None) -> dict:
    """One group (a tile's pixels, or the pooled batch's): ``od_3xp`` (3, P) float32, ``mask_p`` (P,) bool.  NaN rows and a selection count
    of 0 where the contract gives no estimate: per tile fewer than 3 masked-in pixels, pooled fewer than 3 that also pass the OD filter.
    ``plane`` says whether the pixels that pass the filter span a plane (``plane_defined``): where they do not, the row is the reference's
    answer to an ill-posed question and the tests compare counts and identities only, as they do for fallback tiles."""
    sel = np.ascontiguousarray(od_3xp[:, mask_p])
    n_in = int(sel.shape[1])
    passing = sel.min(axis=0) >= so.BETA if n_in else np.zeros(0, dtype=bool)
    kept = int(passing.sum())
    plane = plane_defined(sel[:, passing])
    nothing = {"he": np.full((3, 2), np.nan, F32), "max_c": np.full(2, np.nan, F32), "n_sel": 0, "n_in": n_in, "kept": kept, "plane": plane, "fallback": False, "conc": None}
    if (n_in < 3) if per_tile else (kept < 3):
        return nothing
    p = so.macenko_tile_params(sel.reshape(3, -1, 1), allow_fallback=per_tile, signs=signs)
    return {"he": p["he"], "max_c": p["max_c"], "n_sel": p["n_kept"], "n_in": n_in, "kept": kept, "plane": plane, "fallback": per_tile and kept < 3, "conc": p["conc"]}


def estimate(images: np.ndarray, mask: np.ndarray, *, pooled: bool = False, signs=None) -> list[dict]:
    """Rows of ``group_estimate``: one per tile, or one for the pooled batch.  ``images`` (N, 3, H, W) uint8 / float32, ``mask`` (N, H, W) bool."""
    od = so.optical_density(so.to_unit_float(images))
    n = images.shape[0]
    if pooled:
        return [group_estimate(np.transpose(od, (1, 0, 2, 3)).reshape(3, -1), mask.reshape(-1), per_tile=False, signs=signs)]
    return [group_estimate(od[i].reshape(3, -1), mask[i].reshape(-1), per_tile=True, signs=signs) for i in range(n)]


def fit(images: np.ndarray, mask: np.ndarray, *, signs=None) -> tuple[np.ndarray, np.ndarray]:
    row = estimate(images, mask, pooled=True, signs=signs)[0]
    return row["he"], row["max_c"]


# ------------------------------------------------------------------ the output
def input_level(images: np.ndarray) -> np.ndarray:
    """The background rule's level on the 0-255 scale, float32: the byte itself, or ``x * 255`` formed in float32."""
    if images.dtype == np.uint8:
        return images.astype(F32)
    return images.astype(F32) * F32(255.0)


def transform_levels(images: np.ndarray, stain_matrix, target_max_conc, mask: np.ndarray, *, signs=None) -> tuple[np.ndarray, list[dict]]:
    """(N, 3, H, W) float32 on the 0-255 scale BEFORE the clamp and cast: the tail of ``so.macenko_transform`` (:452-459) on the masked-in
    pixels of every tile with that tile's masked estimate, the input's level elsewhere and on tiles without an estimate."""
    sm = np.asarray(stain_matrix, dtype=F32)
    tmc = np.asarray(target_max_conc, dtype=F32).reshape(-1)
    rows = estimate(images, mask, signs=signs)
    out = input_level(images).copy()
    for i, row in enumerate(rows):
        if row["conc"] is None:
            continue
        scaled = row["conc"] * (tmc / row["max_c"])[:, None]
        od_new = (sm @ scaled).astype(F32)
        rgb = np.clip(so.IO * np.exp(-od_new), F32(0), F32(255))
        flat = out[i].reshape(3, -1)
        flat[:, mask[i].reshape(-1)] = rgb
    return out, rows


def transform(images: np.ndarray, stain_matrix, target_max_conc, mask: np.ndarray, *, signs=None) -> np.ndarray:
    levels, _ = transform_levels(images, stain_matrix, target_max_conc, mask, signs=signs)
    return so.restore_dtype(levels, images.dtype, in_0_255=True)


# ------------------------------------------------------------------ masks
def ones(n: int, h: int, w: int) -> np.ndarray:
    return np.ones((n, h, w), dtype=bool)


def zeros(n: int, h: int, w: int) -> np.ndarray:
    return np.zeros((n, h, w), dtype=bool)


def disc(n: int, h: int, w: int, share: float = 0.6) -> np.ndarray:
    """A centred disc of about ``share`` of the shorter side's square."""
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = share * min(h, w) ** 2 / np.pi
    one = (yy - (h - 1) / 2) ** 2 + (xx - (w - 1) / 2) ** 2 <= r2
    return np.broadcast_to(one, (n, h, w)).copy()


def blocks(n: int, h: int, w: int, s: int = 8, seed: int = 5, share: float = 0.5) -> np.ndarray:
    """Random s x s blocks in or out: they cut through tissue and glass alike."""
    rng = np.random.default_rng(seed)
    coarse = rng.random((n, -(-h // s), -(-w // s))) < share
    return np.repeat(np.repeat(coarse, s, axis=1), s, axis=2)[:, :h, :w].copy()


def exactly(n: int, h: int, w: int, k: int, seed: int = 9) -> np.ndarray:
    """Exactly ``k`` pixels set in every tile."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((n, h * w), dtype=bool)
    for i in range(n):
        mask[i, rng.choice(h * w, size=k, replace=False)] = True
    return mask.reshape(n, h, w)
