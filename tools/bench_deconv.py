"""Cost of the colour-deconvolution calls: `deconv_apply` (three stains, fixed basis, factors) against `Macenko.apply` in own basis with
factors -- the one-launch kernel it is shaped after, over the same bytes -- alternated in ONE process, timed with device events.
    python tools/bench_deconv.py [--out profiles/deconv_bench.json] [--calls 100] [--repeats 5]
Workloads: config 2 (64 x 3 x 512 x 512 float32), 64 x 512 x 512 uint8, 256 x 224 x 224 bfloat16, cut from the real-tissue fixture.
Every apply figure is a ratio to `macenko_apply` OF THE SAME RUN (medians over the alternated windows; min and max reported with them).
`macenko_apply` is also timed against itself (`macenko_apply_again`, A/A): the A/A spread is the larger of the difference of the two
medians and the min-to-max range of its windows.  A row is FLAGGED (exit status 1) when deconv_apply's median exceeds macenko_apply's by
more than twice that spread: same bytes and the same instruction shape should give the same time.  `separate` and `combine` have no
parent to compare with: effective bytes per second (bytes the call must read and write over its median time) only."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import stain_basis, tissue_mask  # noqa: E402
from stainx_amd.backends.torch_hip_backend import DeconvHIP, MacenkoHIP  # noqa: E402
sys.path.insert(0, str(ROOT / "tools"))
from bench_masked import real_batch, window  # noqa: E402  (the batches and the timing window of tools/bench_masked.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deconv_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mac, be = MacenkoHIP(dev), DeconvHIP(dev)
    basis = stain_basis("hed").to(dev)
    he = basis[:, :2].contiguous()      # (3, 2): the same first two stain vectors for the parent
    results, ok = [], True
    for n, size, dtype in ((64, 512, torch.float32), (64, 512, torch.uint8), (256, 224, torch.bfloat16)):
        x = real_batch(n, size, dtype).to(dev)
        mask, _ = tissue_mask(x, 0.8)
        g = torch.Generator().manual_seed(3)
        alpha = (1.0 + 0.05 * (2.0 * torch.rand(n, 3, generator=g) - 1.0)).to(dev)
        beta = (0.05 * (2.0 * torch.rand(n, 3, generator=g) - 1.0)).to(dev)
        a2, b2 = alpha[:, :2].contiguous(), beta[:, :2].contiguous()
        conc = be.separate(x, basis, stains=False, concentrations=True)[1]
        forms = {
            "macenko_apply": lambda: mac.apply(x, he, None, alpha=a2, beta=b2),
            "deconv_apply": lambda: be.apply(x, basis, alpha=alpha, beta=beta),
            "macenko_apply_again": lambda: mac.apply(x, he, None, alpha=a2, beta=b2),
            "deconv_apply_target": lambda: be.apply(x, basis, basis, alpha=alpha, beta=beta),
            "deconv_apply_mask": lambda: be.apply(x, basis, alpha=alpha, beta=beta, masking=(mask, 0.8)),
            "deconv_separate": lambda: be.separate(x, basis, stains=True, concentrations=True),
            "deconv_separate_conc_only": lambda: be.separate(x, basis, stains=False, concentrations=True),
            "deconv_combine": lambda: be.combine(conc, basis, out_dtype=dtype),
        }
        for fn in forms.values():      # warm-up
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for name, fn in forms.items():
                times[name].append(window(fn, args.calls))
        median = {name: float(np.median(values)) for name, values in times.items()}
        elem, pixels = x.element_size(), n * size * size
        moved = {"deconv_separate": pixels * (3 * elem + 9 * elem + 3 * 4), "deconv_separate_conc_only": pixels * (3 * elem + 3 * 4), "deconv_combine": pixels * (3 * 4 + 3 * elem)}
        row = {"shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "calls_per_window": args.calls, "windows": args.repeats}
        for name, values in times.items():
            row[name] = {"median_us": median[name], "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            if name in moved:
                row[name]["effective_GB_per_s"] = moved[name] / median[name] * 1e-3
            else:
                row[name]["ratio_to_macenko_apply"] = median[name] / median["macenko_apply"]
        spread = max(abs(median["macenko_apply"] - median["macenko_apply_again"]), float(np.max(times["macenko_apply"]) - np.min(times["macenko_apply"])))
        row["aa_spread_us"] = spread
        row["deconv_apply_within_twice_the_aa_spread"] = median["deconv_apply"] - median["macenko_apply"] <= 2.0 * spread
        ok = ok and row["deconv_apply_within_twice_the_aa_spread"]
        results.append(row)
        print(json.dumps(row))
        del x, conc
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
