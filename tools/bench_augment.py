#!/usr/bin/env python3
"""Stain augmentation against the transform: device ms per call of three calls on three workloads, one JSON line.

    python tools/bench_augment.py [--steps 200] [--warmup 20] [--workloads config2,real_tiles,config5]

Calls (include/stainx_hip.h):
  own_basis   MacenkoHIP.augment(x, alpha, beta)               -- sx_macenko_augment without a reference: five launches
  normalise   MacenkoHIP.augment(x, alpha, beta, SM, tmc)       -- sx_macenko_augment with the fitted reference: seven launches
  transform   MacenkoHIP.transform(x, SM, tmc, CLASSIC)         -- the four-pass transform the normalise call extends
Workloads: config2 (64x3x512x512 float32 synthetic Beer-Lambert tiles, bench.py's default batches), real_tiles (64 crops of
512 x 512 float32 from tests/golden/g11_real_images.npz, as bench.py --workload real_tiles), config5 (256x3x224x224 bfloat16
synthetic tiles).  bench.py's protocol: warm-up, then K timed steps rotating over two input batches (each with its own factors),
a HIP event after every call on the launch stream; reported: the mean and the minimum of the per-call event times, and wall ms
per step.  One process, no collectives.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from stainx_amd import Macenko, _native, synth  # noqa: E402
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402


def batches_for(name: str) -> tuple[list[torch.Tensor], torch.Tensor]:
    """Two input batches (CPU) and the fit target of a workload."""
    if name == "config2":
        xs = [synth.as_dtype(synth.he_batch(64, 512, 512, seed0=1000 + 64 * b), torch.float32) for b in range(2)]
        return xs, synth.reference_tile(512, 512)
    if name == "config5":
        xs = [synth.as_dtype(synth.he_batch(256, 224, 224, seed0=1000 + 256 * b), torch.bfloat16) for b in range(2)]
        return xs, synth.as_dtype(synth.reference_tile(224, 224), torch.bfloat16)
    if name == "real_tiles":
        imgs = torch.from_numpy(np.load(str(ROOT / "tests" / "golden" / "g11_real_images.npz"))["images_u8"])
        crops = torch.stack([imgs[i, :, y:y + 512, x:x + 512] for i in range(6) for y in range(0, 513, 128) for x in range(0, 513, 128)])
        xs = [synth.as_dtype(crops[torch.arange(b, 150, 150 / 64).long()[:64]], torch.float32) for b in range(2)]
        return xs, imgs[0:1]
    raise ValueError(f"unknown workload {name!r}")


def timed(fn, steps: int, warmup: int) -> dict:
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(steps):
        fn(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return {"ms": round(sum(ms) / len(ms), 4), "ms_min": round(min(ms), 4), "wall_ms_per_step": round(wall / steps * 1e3, 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="config2,real_tiles,config5")
    ap.add_argument("--only", choices=("own_basis", "normalise", "transform"), default=None, help="time this call alone (under a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = MacenkoHIP(dev)
    line = {"tool": "tools/bench_augment.py", "steps": args.steps, "warmup": args.warmup, "batches_rotated": 2, "unit": "device ms per call (HIP events)", "workloads": {}}
    for name in args.workloads.split(","):
        xs_cpu, target = batches_for(name)
        xs = [x.to(dev) for x in xs_cpu]
        n = xs[0].shape[0]
        norm = Macenko(device=dev, backend="torch_hip").fit(target.to(dev))
        sm, tmc = norm._stain_matrix, norm._target_max_conc
        gen = torch.Generator().manual_seed(0)
        fac = [(1.0 + 0.2 * (2 * torch.rand(n, 2, generator=gen) - 1)).to(dev) for _ in range(2)]
        shift = [(0.2 * (2 * torch.rand(n, 2, generator=gen) - 1)).to(dev) for _ in range(2)]
        calls = {
            "own_basis": lambda i: be.augment(xs[i % 2], fac[i % 2], shift[i % 2]),
            "normalise": lambda i: be.augment(xs[i % 2], fac[i % 2], shift[i % 2], sm, tmc),
            "transform": lambda i: be.transform(xs[i % 2], sm, tmc, _extra_flags=_native.MACENKO_CLASSIC),
        }
        rec = {"shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", "")}
        for call, fn in calls.items():
            if args.only is None or args.only == call:
                rec[call] = timed(fn, args.steps, args.warmup)
        if args.only is None:
            rec["own_basis_vs_transform"] = round(rec["own_basis"]["ms"] / rec["transform"]["ms"], 4)
            rec["normalise_vs_transform"] = round(rec["normalise"]["ms"] / rec["transform"]["ms"], 4)
        line["workloads"][name] = rec
        del xs
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
