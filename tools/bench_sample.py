"""Cost of tissue pixel sampling through the C ABI -- sx_sample_pixels, K = 64 x 64 per tile and pooled, under an explicit mask, under the rule
(sx_tissue_mask in front, as stainx_amd.sample_pixels runs it) and without a mask -- on 64 x 3 x 512 x 512 uint8 and float32 batches cut from
the real-tissue fixture.  Every form is alternated in ONE process with sx_tissue_mask on the same batch and with the torch route to the
same pixels (``x.permute(0, 2, 3, 1)[mask]``: a boolean index, whose data-dependent shape synchronises; it neither subsamples nor fixes a
shape) and timed with device events, three windows each.  The torch route is timed with a host clock around calls that end in their own
synchronisation.
    python tools/bench_sample.py [--out profiles/sample_bench.json] [--calls 200] [--repeats 3]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native, synth  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

THRESHOLD = 0.8


def host_window(fn, calls: int) -> float:
    """Mean microseconds per call of a call that synchronises by itself (host clock, the device idle before and after)."""
    torch.cuda.synchronize()
    begin = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) * 1e6 / calls


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sample_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    n, size, k = 64, 512, 64 * 64
    tiles_u8 = real_batch(n, size, torch.uint8)
    results = []
    for dtype in (torch.uint8, torch.float32):
        code = _native.DTYPE_CODES[dtype]
        x = synth.as_dtype(tiles_u8, dtype).to(dev)
        mask = torch.empty((n, size, size), dtype=torch.uint8, device=dev)
        counts = torch.empty((n,), dtype=torch.int64, device=dev)
        pixels = torch.empty((n, 3, k), dtype=dtype, device=dev)
        valid = torch.empty((n, k), dtype=torch.uint8, device=dev)
        taken = torch.empty((n,), dtype=torch.int32, device=dev)
        population = torch.empty((n,), dtype=torch.int64, device=dev)
        ws = torch.empty(lib.sx_sample_workspace_bytes(n, size, size), dtype=torch.uint8, device=dev)

        def check(rc: int) -> None:
            assert rc == 0, _native.last_error()

        def rule() -> None:
            check(lib.sx_tissue_mask(x.data_ptr(), code, n, size, size, 0, THRESHOLD, mask.data_ptr(), counts.data_ptr(), stream))

        def sample(mask_ptr, pooled: int):
            return lambda: check(lib.sx_sample_pixels(x.data_ptr(), code, n, size, size, 0, mask_ptr, pooled, k, 0, pixels.data_ptr(), valid.data_ptr(), taken.data_ptr(),
                                                      population.data_ptr(), ws.data_ptr(), ws.numel(), stream))

        def both(pooled: int):
            inner = sample(mask.data_ptr(), pooled)

            def run() -> None:
                rule()
                inner()

            return run

        rule()
        torch.cuda.synchronize()
        inside = mask != 0
        everything = torch.ones_like(inside)
        nhwc_view = x.permute(0, 2, 3, 1)
        forms = {"tissue_mask": rule, "sample_explicit": sample(mask.data_ptr(), 0), "sample_explicit_pooled": sample(mask.data_ptr(), 1), "sample_rule": both(0), "sample_rule_pooled": both(1),
                 "sample_no_mask": sample(None, 0), "sample_no_mask_pooled": sample(None, 1)}
        torch_forms = {"torch_index_explicit": lambda: nhwc_view[inside].shape[0], "torch_index_rule": lambda: (rule(), nhwc_view[mask != 0].shape[0]),
                       "torch_index_no_mask": lambda: nhwc_view[everything].shape[0]}
        for fn in list(forms.values()) + list(torch_forms.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in list(forms) + list(torch_forms)}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
            for form, fn in torch_forms.items():
                times[form].append(host_window(fn, max(args.calls // 10, 5)))
        forms["sample_explicit"]()
        torch.cuda.synchronize()
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "sample_size": k, "calls_per_window": args.calls, "luminosity_threshold": THRESHOLD,
               "tissue_share": float(inside.float().mean()), "tiles_with_more_than_k": int((population > k).sum()),
               "algorithmic_bytes_explicit": 2 * n * size * size + n * k * (2 * 3 * x.element_size() + 1)}
        for form, values in times.items():
            row[form] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
        mean = {form: row[form]["mean_us"] for form in times}
        row["explicit_to_tissue_mask"] = mean["sample_explicit"] / mean["tissue_mask"]
        row["explicit_pooled_to_tissue_mask"] = mean["sample_explicit_pooled"] / mean["tissue_mask"]
        row["no_mask_to_tissue_mask"] = mean["sample_no_mask"] / mean["tissue_mask"]
        row["torch_index_explicit_to_sample_explicit"] = mean["torch_index_explicit"] / mean["sample_explicit"]
        row["torch_index_rule_to_sample_rule"] = mean["torch_index_rule"] / mean["sample_rule"]
        row["torch_index_no_mask_to_sample_no_mask"] = mean["torch_index_no_mask"] / mean["sample_no_mask"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
