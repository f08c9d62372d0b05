"""Cost of stain quantification: `quantify` (one memset and one streaming launch, no map) against what a user did before it --
`separate(concentrations=True)` followed by three `torch.histc` over the (N, 3, H, W) float32 map -- alternated in ONE process, timed
with device events.
    python tools/bench_quantify.py [--out profiles/quantify_bench.json] [--calls 100] [--repeats 5]
Workloads: config 2 (64 x 3 x 512 x 512 float32), 64 x 512 x 512 uint8, 256 x 224 x 224 bfloat16, cut from the real-tissue fixture,
masked (an explicit mask, the rule's bytes) and unmasked, per tile and pooled.  Every figure is a median over the alternated windows with
its min and max; `ratio_to_separate_histc` is quantify's median over the old path's OF THE SAME RUN.  The old path computes less (three
pooled histograms, no sums, no per-tile sets, no mask); `separate_conc_only` alone is reported too: the map's write is a floor of every
path that goes through it.  `quantify_again` (A/A) gives the spread.  No figure is a gate: the exit status is 0."""
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
from stainx_amd.backends.torch_hip_backend import DeconvHIP  # noqa: E402
sys.path.insert(0, str(ROOT / "tools"))
from bench_masked import real_batch, window  # noqa: E402  (the batches and the timing window of tools/bench_masked.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quantify_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = DeconvHIP(dev)
    basis = stain_basis("hdab").to(dev)
    results = []
    for n, size, dtype in ((64, 512, torch.float32), (64, 512, torch.uint8), (256, 224, torch.bfloat16)):
        x = real_batch(n, size, dtype).to(dev)
        mask, tissue = tissue_mask(x, 0.8)

        def separate_histc():
            conc = be.separate(x, basis, stains=False, concentrations=True)[1]
            return [torch.histc(conc[:, s], bins=256, min=-2.0, max=6.0) for s in range(3)]

        forms = {
            "separate_histc": separate_histc,
            "quantify": lambda: be.quantify(x, basis),
            "quantify_again": lambda: be.quantify(x, basis),
            "quantify_pooled": lambda: be.quantify(x, basis, per_tile=False),
            "quantify_mask": lambda: be.quantify(x, basis, masking=(mask, 0.8)),
            "quantify_mask_pooled": lambda: be.quantify(x, basis, per_tile=False, masking=(mask, 0.8)),
            "separate_conc_only": lambda: be.separate(x, basis, stains=False, concentrations=True),
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
        row = {"shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "calls_per_window": args.calls, "windows": args.repeats,
               "tissue_share": float(tissue.sum()) / pixels}
        for name, values in times.items():
            row[name] = {"median_us": median[name], "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            if name.startswith("quantify"):
                row[name]["ratio_to_separate_histc"] = median[name] / median["separate_histc"]
                row[name]["effective_GB_per_s"] = pixels * (3 * elem + ("mask" in name)) / median[name] * 1e-3      # (bytes the call must read)
        row["aa_spread_us"] = max(abs(median["quantify"] - median["quantify_again"]), float(np.max(times["quantify"]) - np.min(times["quantify"])))
        results.append(row)
        print(json.dumps(row))
        del x, mask
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
