#!/usr/bin/env python3
"""Slide-level Macenko against the per-tile calls: device ms per call on four workloads, one JSON line.

    python tools/bench_apply.py [--steps 200] [--warmup 20] [--workloads config2,off_lattice,u8,config5] [--only CALL]

Calls (include/stainx_hip.h):
  apply              MacenkoHIP.apply(x, he, max_c, SM, tmc)                   -- sx_macenko_apply, a per-tile source (n_sources = N): one launch
  apply_one_source   MacenkoHIP.apply(x, he[0], max_c[0], SM, tmc)             -- one basis for the batch (n_sources = 1)
  apply_factors      MacenkoHIP.apply(x, he, max_c, SM, tmc, alpha=, beta=)    -- normalise and jitter
  estimate           MacenkoHIP.estimate(x)                                    -- sx_macenko_estimate: the four-pass estimate, no output pass
  transform          MacenkoHIP.transform(x, SM, tmc)                          -- the default form (estimate inside the call)
  transform_classic  MacenkoHIP.transform(x, SM, tmc, CLASSIC)                 -- the four-pass form
  augment            MacenkoHIP.augment(x, alpha, beta, SM, tmc)               -- what apply_factors replaces when the source is known
Workloads: config2 (64x3x512x512 float32 synthetic grey levels), off_lattice (64x3x512x512 float32 off the k/255 lattice: resized real
crops, as the reference's example pipeline makes them), u8 (64x3x512x512 uint8), config5 (256x3x224x224 bfloat16).  Protocol as
tools/bench_augment.py: warm-up, then K timed steps rotating over two input batches (and their two sources), a HIP event after every
call on the launch stream; reported: the mean and the minimum of the per-call event times, and wall ms per step.  The sources are
each batch's own per-tile estimates, computed once before the timing.
Diagnostic build (STAINX_DIAG=1): SX_APPLY_SETS=k in the environment sets the pack sets per work item of the apply kernel (A/B of its grid).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from stainx_amd import Macenko, _native, synth  # noqa: E402
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402
from tools.bench_augment import batches_for, timed  # noqa: E402

CALLS = ("apply", "apply_one_source", "apply_factors", "estimate", "transform", "transform_classic", "augment")


def off_lattice_batch(imgs: torch.Tensor, n: int, seed: int) -> torch.Tensor:
    """float32 tiles off the k/255 lattice: random crops of the real images resized to 512 x 512 with antialias."""
    rng = np.random.default_rng(seed)
    tiles = []
    for t in range(n):
        bh, bw = int(rng.integers(300, 1000)), int(rng.integers(300, 1000))
        y, x = int(rng.integers(0, 1024 - bh + 1)), int(rng.integers(0, 1024 - bw + 1))
        crop = imgs[t % 6:t % 6 + 1, :, y:y + bh, x:x + bw].float() / 255.0
        tiles.append(F.interpolate(crop, size=(512, 512), mode="bilinear", antialias=True, align_corners=False))
    return torch.cat(tiles).clamp_(0.0, 1.0).contiguous()


def workload(name: str) -> tuple[list[torch.Tensor], torch.Tensor]:
    if name == "off_lattice":
        imgs = torch.from_numpy(np.load(str(ROOT / "tests" / "golden" / "g11_real_images.npz"))["images_u8"])
        return [off_lattice_batch(imgs, 64, 2024 + b) for b in range(2)], imgs[0:1]
    if name == "u8":
        return [synth.he_batch(64, 512, 512, seed0=1000 + 64 * b) for b in range(2)], synth.reference_tile(512, 512)
    return batches_for(name)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="config2,off_lattice,u8,config5")
    ap.add_argument("--only", choices=CALLS, default=None, help="time this call alone (under a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = MacenkoHIP(dev)
    line = {"tool": "tools/bench_apply.py", "steps": args.steps, "warmup": args.warmup, "batches_rotated": 2, "unit": "device ms per call (HIP events)", "workloads": {}}
    for name in args.workloads.split(","):
        xs_cpu, target = workload(name)
        xs = [x.to(dev) for x in xs_cpu]
        n = xs[0].shape[0]
        norm = Macenko(device=dev, backend="torch_hip").fit(target.to(dev))
        sm, tmc = norm._stain_matrix, norm._target_max_conc
        est = [be.estimate(x) for x in xs]
        he, mc = [e["he"] for e in est], [e["max_c"] for e in est]
        he1, mc1 = [h[0:1].contiguous() for h in he], [m[0:1].contiguous() for m in mc]
        gen = torch.Generator().manual_seed(0)
        fac = [(1.0 + 0.2 * (2 * torch.rand(n, 2, generator=gen) - 1)).to(dev) for _ in range(2)]
        shift = [(0.2 * (2 * torch.rand(n, 2, generator=gen) - 1)).to(dev) for _ in range(2)]
        calls = {
            "apply": lambda i: be.apply(xs[i % 2], he[i % 2], mc[i % 2], sm, tmc),
            "apply_one_source": lambda i: be.apply(xs[i % 2], he1[i % 2], mc1[i % 2], sm, tmc),
            "apply_factors": lambda i: be.apply(xs[i % 2], he[i % 2], mc[i % 2], sm, tmc, alpha=fac[i % 2], beta=shift[i % 2]),
            "estimate": lambda i: be.estimate(xs[i % 2]),
            "transform": lambda i: be.transform(xs[i % 2], sm, tmc),
            "transform_classic": lambda i: be.transform(xs[i % 2], sm, tmc, _extra_flags=_native.MACENKO_CLASSIC),
            "augment": lambda i: be.augment(xs[i % 2], fac[i % 2], shift[i % 2], sm, tmc),
        }
        rec = {"shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", "")}
        for call, fn in calls.items():
            if args.only is None or args.only == call:
                rec[call] = timed(fn, args.steps, args.warmup)
        if args.only is None:
            rec["apply_vs_transform"] = round(rec["apply"]["ms"] / rec["transform"]["ms"], 4)
            rec["apply_vs_transform_classic"] = round(rec["apply"]["ms"] / rec["transform_classic"]["ms"], 4)
            rec["apply_factors_vs_augment"] = round(rec["apply_factors"]["ms"] / rec["augment"]["ms"], 4)
        line["workloads"][name] = rec
        del xs
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
