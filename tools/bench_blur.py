"""Cost of the Gaussian blur through the C ABI -- sx_gaussian_blur with a sigma per tile -- on 64 x 3 x 512 x 512 uint8 and float32 batches
cut from the real-tissue fixture and a 256 x 3 x 224 x 224 bfloat16 batch, at sigma 0.5, 1, 2, 4 (every tile the same) and a mixed row
(sigmas spread evenly over [0.5, 4]), alternated in ONE process with
  sx_hsv_apply        the same bytes in and out, a streaming kernel: what a pass over the batch costs;
  the torch route     element -> float32, reflect padding, two depthwise conv2d (1 x k, then k x 1), round (uint8), cast: what a user has
                      without this kernel -- one sigma per call, so the mixed row has no torch figure;
and timed with device events over windows of back-to-back launches after a warm-up.  The ratios are reported, not gated.  NCHW,
unmasked: the NHWC and the masked forms are not timed here.
    python tools/bench_blur.py [--out profiles/blur_bench.json] [--calls 100] [--torch-calls 10] [--repeats 5]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import HSVAugment, _native  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402


def torch_route(x: torch.Tensor, sigma: float):
    """The closure of the torch route at one sigma; the taps are made once, outside the timed call."""
    radius = min(int(4.0 * sigma + 0.5), 16)
    i = torch.arange(-radius, radius + 1, dtype=torch.float32, device=x.device)
    w = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    w = w / w.sum()
    rows, cols = w.reshape(1, 1, 1, -1).repeat(3, 1, 1, 1), w.reshape(1, 1, -1, 1).repeat(3, 1, 1, 1)

    def run() -> torch.Tensor:
        y = F.pad(x.to(torch.float32), (radius, radius, radius, radius), mode="reflect")
        y = F.conv2d(F.conv2d(y, rows, groups=3), cols, groups=3)
        return torch.round(y).to(torch.uint8) if x.dtype == torch.uint8 else y.to(x.dtype)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "blur_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--torch-calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    results = []

    def check(rc: int) -> None:
        assert rc == 0, _native.last_error()

    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        code = _native.DTYPE_CODES[dtype]
        x = real_batch(n, size, dtype).to(dev)
        out = torch.empty_like(x)
        rows = HSVAugment(0.05, 0.1, 0.1, generator=torch.Generator(device=dev).manual_seed(1)).sample_rows(n, dev).contiguous()
        bytes_moved = 2 * x.numel() * x.element_size()
        for name in ("0.5", "1", "2", "4", "mixed"):
            sigmas = torch.linspace(0.5, 4.0, n, device=dev) if name == "mixed" else torch.full((n,), float(name), device=dev)
            sigmas = sigmas.to(torch.float32).contiguous()
            forms = {"hsv_apply": (lambda: check(lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, rows.data_ptr(), n, 0, stream)), args.calls),
                     "gaussian_blur": (lambda: check(lib.sx_gaussian_blur(x.data_ptr(), out.data_ptr(), code, n, size, size, sigmas.data_ptr(), n, 0, stream)), args.calls)}
            if name != "mixed":
                forms["torch_route"] = (torch_route(x, float(name)), args.torch_calls)
            for fn, _ in forms.values():      # warm-up
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {form: [] for form in forms}
            for _ in range(args.repeats):      # alternated: one window of each form per repeat
                for form, (fn, calls) in forms.items():
                    times[form].append(window(fn, calls))
            row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "sigma": name, "windows": args.repeats, "bytes_read_and_written": bytes_moved}
            for form, values in times.items():
                row[form] = {"calls_per_window": forms[form][1], "median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values)),
                             "gb_per_s_at_median": bytes_moved / float(np.median(values)) / 1e3}
            row["blur_to_hsv_apply"] = row["gaussian_blur"]["median_us"] / row["hsv_apply"]["median_us"]
            if "torch_route" in row:
                row["torch_route_to_blur"] = row["torch_route"]["median_us"] / row["gaussian_blur"]["median_us"]
            results.append(row)
            print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
