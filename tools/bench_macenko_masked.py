"""Cost of the tissue masks for Macenko: the unmasked four-pass (CLASSIC) transform against the masked transform with an explicit mask and
with the rule, `estimate` against the masked estimate, `apply` against the masked apply -- on batches cut from the real-tissue fixture (so
that glass is present), alternated in ONE process, timed with device events.
    python tools/bench_macenko_masked.py [--out profiles/macenko_masked_bench.json] [--calls 100] [--repeats 5]
Every figure is a ratio to the unmasked call OF THE SAME RUN (medians over the alternated windows; the spread is reported with them).
One condition is checked per row: the masked apply does one of the masked transform's launches on a subset of its bytes, so its median
may not exceed the masked transform's of the same run (exit status 1 where it does)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native, synth, tissue_mask  # noqa: E402
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402
sys.path.insert(0, str(ROOT / "tools"))
from bench_masked import real_batch, window  # noqa: E402  (the batches and the timing window of tools/bench_masked.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "macenko_masked_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = MacenkoHIP(dev)
    sm, tmc = be.compute_reference_stain_matrix(synth.reference_tile(256, 256).to(dev))
    classic = _native.MACENKO_CLASSIC
    results, ok = [], True
    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        x = real_batch(n, size, dtype).to(dev)
        mask, counts = tissue_mask(x, 0.8)
        est = be.estimate(x)
        est_m = be.estimate_masked(x, mask)
        forms = {
            "transform": lambda: be.transform(x, sm, tmc, _extra_flags=classic),
            "transform_mask": lambda: be.transform_masked(x, sm, tmc, mask),
            "transform_rule": lambda: be.transform_masked(x, sm, tmc, None, 0.8),
            "estimate": lambda: be.estimate(x),
            "estimate_mask": lambda: be.estimate_masked(x, mask),
            "apply": lambda: be.apply(x, est["he"], est["max_c"], sm, tmc),
            "apply_mask": lambda: be.apply_masked(x, est_m["he"], est_m["max_c"], sm, tmc, mask),
        }
        for fn in forms.values():      # warm-up
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for name, fn in forms.items():
                times[name].append(window(fn, args.calls))
        row = {"shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "tissue_share": float(counts.sum().item()) / (n * size * size),
               "calls_per_window": args.calls, "windows": args.repeats}
        median = {name: float(np.median(values)) for name, values in times.items()}
        for name, values in times.items():
            base = median[name.split("_")[0]]      # the unmasked call of the same kind, same run
            row[name] = {"median_us": median[name], "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_unmasked": median[name] / base}
        row["apply_mask_not_slower_than_transform_mask"] = median["apply_mask"] <= median["transform_mask"]
        ok = ok and row["apply_mask_not_slower_than_transform_mask"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
