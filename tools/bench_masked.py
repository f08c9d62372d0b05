"""Cost of the tissue masks: the unmasked statistics="tile" call, the rule call and the explicit-mask call of Reinhard and histogram matching
on batches cut from the real-tissue fixture (so that background is present), alternated in ONE process, timed with device events.
    python tools/bench_masked.py [--out profiles/masked_bench.json] [--calls 200] [--repeats 3]
Every figure is compared with the unmasked call OF THE SAME RUN; the spread of the repeats is reported with the means."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import synth, tissue_mask  # noqa: E402
from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP  # noqa: E402


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "masked_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = synth.reference_tile(256, 256).to(dev)
    configs = [("reinhard", 64, 512, torch.float32), ("reinhard", 64, 512, torch.uint8), ("reinhard", 256, 224, torch.bfloat16), ("hm", 64, 1024, torch.uint8)]
    results = []
    for method, n, size, dtype in configs:
        x = real_batch(n, size, dtype).to(dev)
        mask, counts = tissue_mask(x, 0.8)
        if method == "reinhard":
            be = ReinhardHIP(dev)
            rm, rs = be.compute_reference_mean_std(ref)
            forms = {"unmasked": lambda: be.transform_tiles(x, rm, rs), "rule": lambda: be.transform_masked(x, rm, rs, None, 0.8, per_tile=True),
                     "mask": lambda: be.transform_masked(x, rm, rs, mask, 0.8, per_tile=True)}
        else:
            be = HistogramMatchingHIP(dev)
            hists = be.compute_reference_histograms(ref)
            forms = {"unmasked": lambda: be.transform_tiles(x, hists), "rule": lambda: be.transform_masked(x, hists, None, 0.8, per_tile=True),
                     "mask": lambda: be.transform_masked(x, hists, mask, 0.8, per_tile=True)}
        for fn in forms.values():      # warm-up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for name, fn in forms.items():
                times[name].append(window(fn, args.calls))
        row = {"method": method, "shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "tissue_share": float(counts.sum().item()) / (n * size * size),
               "calls_per_window": args.calls}
        base = float(np.mean(times["unmasked"]))
        for name, values in times.items():
            row[name] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_unmasked": float(np.mean(values)) / base}
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
