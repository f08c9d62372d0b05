#!/usr/bin/env python3
"""Per-tile Reinhard / histogram matching against the pooled calls and against the loop of one-tile calls: device ms per call, one JSON line.

    python tools/bench_per_tile.py [--steps 100] [--warmup 10] [--workloads reinhard_f32,reinhard_u8,reinhard_bf16,hm_u8] [--only CALL] [--out FILE]

Calls (include/stainx_hip.h):
  pooled    ReinhardHIP.transform / HistogramMatchingHIP.transform           -- statistics pooled over the batch (the *_ready entry points)
  per_tile  ReinhardHIP.transform_tiles / HistogramMatchingHIP.transform_tiles -- sx_reinhard_transform_tiles / sx_hm_transform_tiles
  loop      the pooled call on x[i:i+1] for every tile                         -- what a user writes without the per-tile calls
  apply     ReinhardHIP.apply_statistics(x, tile statistics)                   -- sx_reinhard_apply_stats, n_sources = N (Reinhard only)
  apply_one ReinhardHIP.apply_statistics(x, one row)                           -- n_sources = 1 (Reinhard only)
Workloads: reinhard_f32 / reinhard_u8 (64x3x512x512), reinhard_bf16 (256x3x224x224), hm_u8 (64x3x1024x1024 uint8).  Protocol as
tools/bench_augment.py: warm-up, then K timed steps rotating over two input batches, a HIP event after every call on the launch stream;
reported: the mean and the minimum of the per-call event times, and wall ms per step.  `pooled` is timed twice, first and last, and
`pooled_spread` is the relative difference of the two means: the run's own measure of what a ratio near 1 means.  --loop-steps bounds the
steps of `loop` (N launches-bound calls per step).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from bench import source_hash  # noqa: E402
from stainx_amd import synth  # noqa: E402
from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP  # noqa: E402
from tools.bench_augment import timed  # noqa: E402

CALLS = ("pooled", "per_tile", "loop", "apply", "apply_one")
WORKLOADS = {"reinhard_f32": ("reinhard", 64, 512, torch.float32), "reinhard_u8": ("reinhard", 64, 512, torch.uint8),
             "reinhard_bf16": ("reinhard", 256, 224, torch.bfloat16), "hm_u8": ("hm", 64, 1024, torch.uint8)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--tiles", type=int, default=None, help="tiles per batch instead of the workload's own (launch counts under a kernel trace)")
    ap.add_argument("--side", type=int, default=None, help="tile height and width instead of the workload's own")
    ap.add_argument("--only", choices=CALLS, default=None, help="time this call alone (under a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"tool": "tools/bench_per_tile.py", "steps": args.steps, "warmup": args.warmup, "loop_steps": args.loop_steps, "batches_rotated": 2,
            "unit": "device ms per call (HIP events)", "kernel_source_hash": source_hash(), "workloads": {}}
    for name in args.workloads.split(","):
        kind, n, side, dtype = WORKLOADS[name]
        n, side = args.tiles or n, args.side or side
        distinct = min(n, 256)      # (more tiles than that, --tiles: the distinct ones repeated -- the timing does not depend on it)
        xs = [synth.as_dtype(synth.he_batch(distinct, side, side, seed0=1000 + n * b, scale_step=0.01), dtype)[torch.arange(n) % distinct].to(dev) for b in range(2)]
        target = synth.as_dtype(synth.reference_tile(side, side), dtype).to(dev)
        if kind == "reinhard":
            be = ReinhardHIP(dev)
            ref = be.compute_reference_mean_std(target)
            stats = [be.tile_statistics(x) for x in xs]
            one = [(m[:1].contiguous(), s[:1].contiguous()) for m, s in stats]
            calls = {"pooled": lambda i: be.transform(xs[i % 2], *ref),
                     "per_tile": lambda i: be.transform_tiles(xs[i % 2], *ref),
                     "loop": lambda i: [be.transform(xs[i % 2][t:t + 1], *ref) for t in range(n)],
                     "apply": lambda i: be.apply_statistics(xs[i % 2], *stats[i % 2], *ref),
                     "apply_one": lambda i: be.apply_statistics(xs[i % 2], *one[i % 2], *ref)}
        else:
            be = HistogramMatchingHIP(dev)
            hists = be.compute_reference_histograms(target)
            calls = {"pooled": lambda i: be.transform(xs[i % 2], hists),
                     "per_tile": lambda i: be.transform_tiles(xs[i % 2], hists),
                     "loop": lambda i: [be.transform(xs[i % 2][t:t + 1], hists) for t in range(n)]}
        rec = {"shape": list(xs[0].shape), "dtype": str(dtype).replace("torch.", "")}
        for call, fn in calls.items():
            if args.only is None or args.only == call:
                rec[call] = timed(fn, min(args.steps, args.loop_steps) if call == "loop" else args.steps, 2 if call == "loop" else args.warmup)
        if args.only is None:
            rec["pooled_again"] = timed(calls["pooled"], args.steps, args.warmup)
            rec["pooled_spread"] = round(abs(rec["pooled_again"]["ms"] - rec["pooled"]["ms"]) / rec["pooled"]["ms"], 4)
            rec["per_tile_vs_pooled"] = round(rec["per_tile"]["ms"] / rec["pooled"]["ms"], 4)
            rec["per_tile_vs_loop"] = round(rec["per_tile"]["ms"] / rec["loop"]["ms"], 4)
            rec["per_tile_faster_than_loop"] = rec["per_tile"]["ms"] < rec["loop"]["ms"]
        line["workloads"][name] = rec
        del xs
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
