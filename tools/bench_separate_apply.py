"""Cost of separation and augmentation with a given source basis and under tissue masks: `separate` against `separate_apply`,
`separate_masked` and `separate_apply_masked`; `augment` against `augment_masked` and the given-basis `apply` with factors -- alternated
in ONE process, timed with device events.
    python tools/bench_separate_apply.py [--out profiles/separate_apply_bench.json] [--calls 100] [--repeats 5]
Workloads: config 2 (64 x 3 x 512 x 512 float32), 64 x 512 x 512 uint8, 256 x 224 x 224 bfloat16, cut from the real-tissue fixture (so that
glass is present).  Every figure is a ratio to `separate` (the separation rows) or to `augment` (the augmentation rows) OF THE SAME RUN
(medians over the alternated windows; the spread is reported with them).  One condition is checked per row: separate_apply does a strict
subset of separate's work -- its one streaming pass without the estimate's launches -- so its median may not exceed separate's of the
same run (exit status 1 where it does)."""
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
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402
sys.path.insert(0, str(ROOT / "tools"))
from bench_masked import real_batch, window  # noqa: E402  (the batches and the timing window of tools/bench_masked.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "separate_apply_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = MacenkoHIP(dev)
    sm, tmc = be.compute_reference_stain_matrix(synth.reference_tile(256, 256).to(dev))
    results, ok = [], True
    for n, size, dtype in ((64, 512, torch.float32), (64, 512, torch.uint8), (256, 224, torch.bfloat16)):
        x = real_batch(n, size, dtype).to(dev)
        mask, counts = tissue_mask(x, 0.8)
        est = be.estimate(x)
        est_m = be.estimate_masked(x, mask)
        g = torch.Generator().manual_seed(3)
        alpha = (1.0 + 0.2 * (2.0 * torch.rand(n, 2, generator=g) - 1.0)).to(dev)
        beta = (0.2 * (2.0 * torch.rand(n, 2, generator=g) - 1.0)).to(dev)
        forms = {
            "separate": lambda: be.separate(x, sm, tmc),
            "separate_apply": lambda: be.separate_apply(x, est["he"], est["max_c"], sm, tmc),
            "separate_mask": lambda: be.separate_masked(x, sm, tmc, mask),
            "separate_rule": lambda: be.separate_masked(x, sm, tmc, None, 0.8),
            "separate_apply_mask": lambda: be.separate_apply_masked(x, est_m["he"], est_m["max_c"], sm, tmc, mask),
            "separate_conc_only": lambda: be.separate(x, sm, tmc, stains=False, concentrations=True),
            "separate_apply_conc_only": lambda: be.separate_apply(x, est["he"], est["max_c"], sm, tmc, stains=False, concentrations=True),
            "augment": lambda: be.augment(x, alpha, beta, sm, tmc),
            "augment_mask": lambda: be.augment_masked(x, alpha, beta, sm, tmc, mask),
            "augment_rule": lambda: be.augment_masked(x, alpha, beta, sm, tmc, None, 0.8),
            "augment_given": lambda: be.apply(x, est["he"], est["max_c"], sm, tmc, alpha=alpha, beta=beta),
            "augment_given_mask": lambda: be.apply_masked(x, est_m["he"], est_m["max_c"], sm, tmc, mask, alpha=alpha, beta=beta),
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
            base = median[name.split("_")[0]]      # `separate` or `augment` of the same run
            row[name] = {"median_us": median[name], "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_" + name.split("_")[0]: median[name] / base}
        row["separate_apply_not_slower_than_separate"] = median["separate_apply"] <= median["separate"]
        ok = ok and row["separate_apply_not_slower_than_separate"]
        results.append(row)
        print(json.dumps(row))
        del x
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
