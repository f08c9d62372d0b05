#!/usr/bin/env python3
"""Stain separation against what it replaces: device ms per call of five calls on three workloads, one JSON line.

    python tools/bench_separate.py [--steps 200] [--warmup 20] [--workloads config2,real_tiles,config5] [--only CALL]

Calls (include/stainx_hip.h):
  own_basis     MacenkoHIP.separate(x)                      -- sx_macenko_separate, H and E images in each tile's own basis: five launches
  normalised    MacenkoHIP.separate(x, SM, tmc)             -- the same with the fitted reference (torchstain's H and E): seven launches
  conc_only     MacenkoHIP.separate(x, SM, tmc, stains=False, concentrations=True)  -- the (N, 2, H, W) float32 maps only
  two_augments  MacenkoHIP.augment(x, (1, 0), 0, SM, tmc) + augment(x, (0, 1), 0, SM, tmc)  -- the composition `normalised` replaces
  transform     MacenkoHIP.transform(x, SM, tmc, CLASSIC)   -- the four-pass transform
Workloads and protocol as tools/bench_augment.py: config2 (64x3x512x512 float32 synthetic tiles), real_tiles (64 crops of 512 x 512
float32 from tests/golden/g11_real_images.npz), config5 (256x3x224x224 bfloat16); warm-up, then K timed steps rotating over two input
batches, a HIP event after every call on the launch stream; reported: the mean and the minimum of the per-call event times, and wall
ms per step.
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

from stainx_amd import Macenko, _native  # noqa: E402
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402
from tools.bench_augment import batches_for, timed  # noqa: E402

CALLS = ("own_basis", "normalised", "conc_only", "two_augments", "transform")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="config2,real_tiles,config5")
    ap.add_argument("--only", choices=CALLS, default=None, help="time this call alone (under a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = MacenkoHIP(dev)
    line = {"tool": "tools/bench_separate.py", "steps": args.steps, "warmup": args.warmup, "batches_rotated": 2, "unit": "device ms per call (HIP events)", "workloads": {}}
    for name in args.workloads.split(","):
        xs_cpu, target = batches_for(name)
        xs = [x.to(dev) for x in xs_cpu]
        n = xs[0].shape[0]
        norm = Macenko(device=dev, backend="torch_hip").fit(target.to(dev))
        sm, tmc = norm._stain_matrix, norm._target_max_conc
        zeros = torch.zeros(n, 2, device=dev)
        e_h = torch.tensor([[1.0, 0.0]], device=dev).expand(n, 2).contiguous()
        e_e = torch.tensor([[0.0, 1.0]], device=dev).expand(n, 2).contiguous()
        calls = {
            "own_basis": lambda i: be.separate(xs[i % 2]),
            "normalised": lambda i: be.separate(xs[i % 2], sm, tmc),
            "conc_only": lambda i: be.separate(xs[i % 2], sm, tmc, stains=False, concentrations=True),
            "two_augments": lambda i: (be.augment(xs[i % 2], e_h, zeros, sm, tmc), be.augment(xs[i % 2], e_e, zeros, sm, tmc)),
            "transform": lambda i: be.transform(xs[i % 2], sm, tmc, _extra_flags=_native.MACENKO_CLASSIC),
        }
        rec = {"shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", "")}
        for call, fn in calls.items():
            if args.only is None or args.only == call:
                rec[call] = timed(fn, args.steps, args.warmup)
        if args.only is None:
            rec["normalised_vs_two_augments"] = round(rec["normalised"]["ms"] / rec["two_augments"]["ms"], 4)
            rec["normalised_vs_transform"] = round(rec["normalised"]["ms"] / rec["transform"]["ms"], 4)
        line["workloads"][name] = rec
        del xs
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
