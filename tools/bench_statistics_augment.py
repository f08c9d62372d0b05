"""Cost of statistics-space augmentation through the C ABI -- sx_deconv_moments (per tile, pooled, masked), sx_reinhard_apply_targets -- and
of StatisticsAugment.forward in both spaces, on 64 x 3 x 512 x 512 uint8 and float32 batches cut from the real-tissue fixture and a
256 x 3 x 224 x 224 bfloat16 batch.  Every call is alternated in ONE process with the calls it is compared with, timed with device events:
    sx_deconv_moments            against sx_deconv_quantify (the same loop with the LDS histogram) and sx_tissue_mask (a bare streaming read)
    sx_reinhard_apply_targets    against sx_reinhard_apply_stats (the same body with one target row)
    forward, space="lab"         against Reinhard(statistics="tile").transform (statistics pass + apply pass)
    forward, space="hed"         against HEDAugment (one apply launch, no statistics)
    both forwards also as ONE replay of a captured graph (explicit targets): the chain's device time without the host's launch costs
    python tools/bench_statistics_augment.py [--out profiles/statistics_augment_bench.json] [--calls 200] [--repeats 3]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import ColorDeconvolution, HEDAugment, Reinhard, StatisticsAugment, StatisticsDistribution, _native, stain_basis  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "statistics_augment_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    basis = stain_basis("hed").to(dev)
    results = []
    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        code = _native.DTYPE_CODES[dtype]
        x = real_batch(n, size, dtype).to(dev)
        out = torch.empty_like(x)
        moments, pooled, hist = (torch.empty(shape, dtype=torch.int64, device=dev) for shape in ((n, 7), (1, 7), (n, 772)))
        mask = torch.empty((n, size, size), dtype=torch.uint8, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        reinhard = Reinhard(device=dev, statistics="tile").fit(x[:1])
        own = reinhard.estimate(x)
        src_mean, src_std = own.mean.contiguous(), own.std.contiguous()
        tgt_mean, tgt_std = src_mean.flip(0).contiguous(), src_std.flip(0).contiguous()      # (tile t gets the statistics of tile n - 1 - t)
        ref_mean, ref_std = reinhard._reference_mean.to(dev).float().contiguous(), reinhard._reference_std.to(dev).float().contiguous()
        cd = ColorDeconvolution("hed", device=dev, normalize_to_0_1=True)
        lab = StatisticsAugment(StatisticsDistribution.fit(own), "lab", generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        hed = StatisticsAugment(StatisticsDistribution.fit(cd.estimate(x)), "hed", generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        jitter = HEDAugment(device=dev, generator=torch.Generator(device=dev).manual_seed(1))

        def captured(module, targets):
            """One replay of ``module(x, targets=...)`` captured in a graph: the chain's device time without the host's launch costs."""
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                module(x, targets=targets)
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                module(x, targets=targets)
            return graph

        hed_own = cd.estimate(x)._mean_std()
        lab_graph = captured(lab, (tgt_mean, tgt_std))
        hed_graph = captured(hed, (hed_own[0].float().flip(0).contiguous(), hed_own[1].float().flip(0).contiguous()))

        def check(rc: int) -> None:
            assert rc == 0, _native.last_error()

        forms = {"tissue_mask": lambda: check(lib.sx_tissue_mask(x.data_ptr(), code, n, size, size, 0, 0.8, mask.data_ptr(), counts.data_ptr(), stream)),
                 "deconv_quantify": lambda: check(lib.sx_deconv_quantify(x.data_ptr(), code, n, size, size, basis.data_ptr(), 1, 5, 64, 1, hist.data_ptr(), 0, stream)),
                 "deconv_moments": lambda: check(lib.sx_deconv_moments(x.data_ptr(), code, n, size, size, basis.data_ptr(), 1, 1, moments.data_ptr(), 0, stream)),
                 "deconv_moments_pooled": lambda: check(lib.sx_deconv_moments(x.data_ptr(), code, n, size, size, basis.data_ptr(), 1, 0, pooled.data_ptr(), 0, stream)),
                 "deconv_moments_masked": lambda: check(lib.sx_deconv_moments_masked(x.data_ptr(), code, n, size, size, basis.data_ptr(), 1, 1, moments.data_ptr(), mask.data_ptr(), 0, stream)),
                 "reinhard_apply_stats": lambda: check(lib.sx_reinhard_apply_stats(x.data_ptr(), out.data_ptr(), code, n, size, size, src_mean.data_ptr(), src_std.data_ptr(), n,
                                                                                   ref_mean.data_ptr(), ref_std.data_ptr(), stream)),
                 "reinhard_apply_targets": lambda: check(lib.sx_reinhard_apply_targets(x.data_ptr(), out.data_ptr(), code, n, size, size, src_mean.data_ptr(), src_std.data_ptr(), n,
                                                                                       tgt_mean.data_ptr(), tgt_std.data_ptr(), n, stream)),
                 "reinhard_tile_transform": lambda: reinhard.transform(x),
                 "forward_lab": lambda: lab(x),
                 "hed_augment": lambda: jitter(x),
                 "forward_hed": lambda: hed(x),
                 "forward_lab_captured": lab_graph.replay,      # (explicit targets: the estimate, the factors on the device, the apply launch)
                 "forward_hed_captured": hed_graph.replay}
        for fn in forms.values():      # warm-up (the mask is in `mask` before the masked pass is timed)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "calls_per_window": args.calls, "tissue_share": float(mask.float().mean())}
        for form, values in times.items():
            row[form] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
        mean = {form: row[form]["mean_us"] for form in forms}
        for form in ("deconv_moments", "deconv_moments_pooled", "deconv_moments_masked"):
            row[form + "_to_quantify"] = mean[form] / mean["deconv_quantify"]
            row[form + "_to_tissue_mask"] = mean[form] / mean["tissue_mask"]
        row["apply_targets_to_apply_stats"] = mean["reinhard_apply_targets"] / mean["reinhard_apply_stats"]
        row["forward_lab_to_reinhard_tile_transform"] = mean["forward_lab"] / mean["reinhard_tile_transform"]
        row["forward_hed_to_hed_augment"] = mean["forward_hed"] / mean["hed_augment"]
        row["forward_lab_captured_to_reinhard_tile_transform"] = mean["forward_lab_captured"] / mean["reinhard_tile_transform"]
        row["forward_hed_captured_to_hed_augment"] = mean["forward_hed_captured"] / mean["hed_augment"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
