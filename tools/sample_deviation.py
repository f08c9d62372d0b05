"""How far a Macenko estimate on a SAMPLE of a tile's tissue pixels lies from the estimate on all of them.  CPU only: the numpy restatement
of the sampling rule (tests/_sample_numpy.py) and the restated masked Macenko estimate built on the oracle (tests/_macenko_masked_numpy.py); no
GPU, no library.  On the twenty 512 x 512 tissue quadrants of the real fixture (tests/golden/cases.py: real_quadrants_512; the tiles
tests/golden/g11_real_tissue.npz was computed from), under the luminosity mask at 0.8, for K = 1024, 4096, 16384 at offset 0:
    the angle between the stain vectors (hematoxylin, eosin) from the sample and from the full tile, in degrees;
    the relative difference of the two maxC;
and the same for ONE sample pooled over the twenty tiles against the pooled estimate of all their tissue.  A description of the method,
not a bound: nothing is gated on these figures.
    python tools/sample_deviation.py [--out profiles/sample_deviation.json]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import _macenko_masked_numpy as mm  # noqa: E402
from tests import _masked_numpy as mn  # noqa: E402
from tests import _sample_numpy as sn  # noqa: E402
from tests.golden.cases import real_quadrants_512  # noqa: E402

SIZES = (1024, 4096, 16384)


def angles_deg(he_a: np.ndarray, he_b: np.ndarray) -> list[float]:
    """The angle between corresponding columns (unit stain vectors) of two (3, 2) bases."""
    out = []
    for c in range(2):
        a, b = he_a[:, c].astype(np.float64), he_b[:, c].astype(np.float64)
        cos = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
        out.append(float(np.degrees(np.arccos(min(1.0, max(-1.0, cos))))))
    return out


def compare(full: dict, part: dict) -> dict:
    h, e = angles_deg(full["he"], part["he"])
    rel = np.abs(part["max_c"].astype(np.float64) / full["max_c"].astype(np.float64) - 1.0)
    return {"angle_h_deg": h, "angle_e_deg": e, "max_c_rel_h": float(rel[0]), "max_c_rel_e": float(rel[1])}


def summary(rows: list[dict]) -> dict:
    out = {}
    for key in ("angle_h_deg", "angle_e_deg", "max_c_rel_h", "max_c_rel_e"):
        values = np.array([r[key] for r in rows])
        out[key] = {"median": float(np.median(values)), "max": float(values.max())}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sample_deviation.json"))
    args = ap.parse_args()
    images = mn.real_images()[0].numpy()
    quads = np.stack([images[i, :, y:y + 512, x:x + 512] for i, y, x in real_quadrants_512()])
    mask = mn.rule_mask(quads)[0]
    full_rows = mm.estimate(quads, mask, signs="positive_sum")
    full_pooled = mm.estimate(quads, mask, pooled=True, signs="positive_sum")[0]
    result = {"tiles": int(quads.shape[0]), "tile_shape": [3, 512, 512], "mask": "luminosity, 0.8", "offset": 0, "tissue_pixels_per_tile": [int(r["n_in"]) for r in full_rows], "sizes": {}}
    for k in SIZES:
        pixels, valid, taken, _ = sn.sample_pixels(quads, (1, k), mask)
        rows = [compare(full, part) | {"tile": t, "taken": int(taken[t])} for t, (full, part) in enumerate(zip(full_rows, mm.estimate(pixels, valid != 0, signs="positive_sum")))]
        pooled_pixels, pooled_valid, pooled_taken, _ = sn.sample_pixels(quads, (1, k), mask, pooled=True)
        pooled = compare(full_pooled, mm.estimate(pooled_pixels, pooled_valid != 0, pooled=True, signs="positive_sum")[0]) | {"taken": int(pooled_taken[0])}
        result["sizes"][str(k)] = {"per_tile": summary(rows), "pooled_over_the_tiles": pooled, "tiles": rows}
        print(json.dumps({"K": k, "per_tile": summary(rows), "pooled_over_the_tiles": pooled}))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
