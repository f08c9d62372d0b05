"""Cost of the HSV jitter through the C ABI -- sx_hsv_apply with a row per tile -- on 64 x 3 x 512 x 512 uint8 and float32 batches cut from
the real-tissue fixture and a 256 x 3 x 224 x 224 bfloat16 batch, alternated in ONE process with sx_deconv_apply with factors (HEDAugment's
launch: the same read, the same write, three logarithms and three exponentials where this one has two quotients) and timed with device
events over windows of back-to-back launches after a warm-up.  The ratio to sx_deconv_apply is reported, not gated.  NCHW, unmasked:
the NHWC and the masked forms are not timed here.
    python tools/bench_hsv.py [--out profiles/hsv_bench.json] [--calls 200] [--repeats 5]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import HSVAugment, _native, stain_basis  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hsv_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    basis = stain_basis("hed").to(dev).contiguous()
    results = []
    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        code = _native.DTYPE_CODES[dtype]
        x = real_batch(n, size, dtype).to(dev)
        out = torch.empty_like(x)
        gen = torch.Generator(device=dev).manual_seed(1)
        rows = HSVAugment(0.05, 0.1, 0.1, saturation_shift=0.02, value_shift=0.02, generator=gen).sample_rows(n, dev).contiguous()
        alpha = (1.0 + 0.05 * (2.0 * torch.rand((n, 3), generator=gen, device=dev) - 1.0)).contiguous()
        beta = (0.05 * (2.0 * torch.rand((n, 3), generator=gen, device=dev) - 1.0)).contiguous()

        def check(rc: int) -> None:
            assert rc == 0, _native.last_error()

        forms = {"deconv_apply": lambda: check(lib.sx_deconv_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, basis.data_ptr(), 1, None, 0, alpha.data_ptr(), beta.data_ptr(), 0, stream)),
                 "hsv_apply": lambda: check(lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, rows.data_ptr(), n, 0, stream))}
        for fn in forms.values():      # warm-up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        bytes_moved = 2 * x.numel() * x.element_size()
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "calls_per_window": args.calls, "windows": args.repeats, "bytes_read_and_written": bytes_moved}
        for form, values in times.items():
            row[form] = {"median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values)), "gb_per_s_at_median": bytes_moved / float(np.median(values)) / 1e3}
        row["hsv_to_deconv_apply"] = row["hsv_apply"]["median_us"] / row["deconv_apply"]["median_us"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
