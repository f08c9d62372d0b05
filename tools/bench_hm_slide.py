"""Cost of slide-level histogram matching: ``apply`` with GIVEN lookup tables (one launch) against the statistics="tile" and "batch" transforms
(clear, histogram pass, table launch, apply pass) of the same run, on batches cut from the real-tissue fixture, unmasked and with the
luminosity rule; the estimate and table calls beside them.  ONE process, device events, the forms alternated window by window.
    python tools/bench_hm_slide.py [--out profiles/hm_slide_bench.json] [--calls 200] [--repeats 5]
Every figure is compared with the transform OF THE SAME RUN (medians over the repeats; their spread is reported).  The condition: a
given-tables call does one of the transform's three launches and moves a subset of its bytes, so its median may not exceed the
transform's -- ``condition_holds`` per row, and the exit status is 1 when a row misses it."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import synth  # noqa: E402
from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP  # noqa: E402

THRESHOLD = 0.8


def real_batch(n: int, size: int, dtype: torch.dtype) -> torch.Tensor:
    """n tiles of size x size cut from the six 1024 x 1024 images of the fixture, walking over images and offsets."""
    images = torch.from_numpy(np.load(ROOT / "tests" / "golden" / "g11_real_images.npz")["images_u8"])
    per_side = 1024 // size
    tiles = []
    for k in range(n):
        img, cell = k % 6, (k // 6) % (per_side * per_side)
        r, c = (cell // per_side) * size, (cell % per_side) * size
        tiles.append(images[img, :, r:r + size, c:c + size])
    return synth.as_dtype(torch.stack(tiles).contiguous(), dtype)


def window(fn, calls: int) -> float:
    """Mean microseconds per call over one window of `calls` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / calls


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hm_slide_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="index of the one configuration to run (kernel traces)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = synth.reference_tile(256, 256).to(dev)
    configs = [(64, 512, torch.float32), (64, 512, torch.uint8), (64, 1024, torch.uint8), (256, 224, torch.bfloat16)]
    if args.only is not None:
        configs = [configs[args.only]]
    results, ok = [], True
    for n, size, dtype in configs:
        x = real_batch(n, size, dtype).to(dev)
        be = HistogramMatchingHIP(dev)
        hists = be.compute_reference_histograms(ref)
        for rule in (False, True):
            per_tile = be.lookup_tables(*be.estimate_histograms(x, per_tile=True, masked=rule, luminosity_threshold=THRESHOLD), hists)
            counts, pixels = be.estimate_histograms(x, per_tile=False, masked=rule, luminosity_threshold=THRESHOLD)
            pooled = be.lookup_tables(counts, pixels, hists)
            counts_n, pixels_n = counts.expand(n, 3, 256).contiguous(), pixels.expand(n).contiguous()
            if rule:
                forms = {"transform_tile": lambda: be.transform_masked(x, hists, None, THRESHOLD, per_tile=True),
                         "transform_batch": lambda: be.transform_masked(x, hists, None, THRESHOLD, per_tile=False),
                         "apply_tile_tables": lambda: be.apply_tables_masked(x, per_tile, None, THRESHOLD),
                         "apply_one_table": lambda: be.apply_tables_masked(x, pooled, None, THRESHOLD)}
            else:
                forms = {"transform_tile": lambda: be.transform_tiles(x, hists), "transform_batch": lambda: be.transform(x, hists),
                         "apply_tile_tables": lambda: be.apply_tables(x, per_tile), "apply_one_table": lambda: be.apply_tables(x, pooled)}
            forms["estimate_tile"] = lambda: be.estimate_histograms(x, per_tile=True, masked=rule, luminosity_threshold=THRESHOLD)
            forms["lookup_tables_tile"] = lambda: be.lookup_tables(counts_n, pixels_n, hists)
            for fn in forms.values():      # warm-up
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in forms}
            for _ in range(args.repeats):      # alternated: one window of each form per repeat
                for name, fn in forms.items():
                    times[name].append(window(fn, args.calls))
            row = {"shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "mask": "luminosity" if rule else None, "calls_per_window": args.calls,
                   "repeats": args.repeats}
            for name, values in times.items():
                row[name] = {"median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            tile, batch = row["transform_tile"]["median_us"], row["transform_batch"]["median_us"]
            row["apply_tile_tables"]["ratio_to_transform_tile"] = row["apply_tile_tables"]["median_us"] / tile
            row["apply_one_table"]["ratio_to_transform_batch"] = row["apply_one_table"]["median_us"] / batch
            row["condition_holds"] = bool(row["apply_tile_tables"]["median_us"] <= tile and row["apply_one_table"]["median_us"] <= batch)
            ok = ok and row["condition_holds"]
            results.append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "condition_holds": ok, "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
