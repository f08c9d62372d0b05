"""Cost of focus measurement through the C ABI: sx_grey_map, sx_focus_statistics with one cell per tile, 64 x 64 and 16 x 16 cells, masked
and pooled, and focus_mask end to end, on 64 x 3 x 512 x 512 uint8 and float32 batches and a 256 x 3 x 224 x 224 bfloat16 batch cut from
the real-tissue fixture; alternated in ONE process with sx_saturation_map and sx_luminosity_histogram, which read the same bytes, with
sx_median_filter_u8 at 3 x 3, the other staged stencil, and with the torch route (a float grey map, two conv2d, var and mean); timed with
device events.
    python tools/bench_focus.py [--out profiles/focus_bench.json] [--calls 200] [--repeats 3]
The yardstick is the ratio to sx_luminosity_histogram OF THE SAME RUN -- one read of the tile with integer adds; the spread of the repeats is
reported with the means.  Also records the size of the library."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native, focus_mask, tissue_mask  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

CONFIGS = ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16))
MIN_VARIANCE = 400.0


def torch_route(images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """What users do today in torch: a float grey map, the Laplacian and the Sobel pair as conv2d on a reflect-padded map, var and mean per tile."""
    x = images.to(torch.float32)
    grey = (0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3])
    padded = torch.nn.functional.pad(grey, (1, 1, 1, 1), mode="reflect")
    lap = torch.nn.functional.conv2d(padded, torch_route.laplace)
    sob = torch.nn.functional.conv2d(padded, torch_route.sobel)
    return lap.var(dim=(1, 2, 3), unbiased=False), (sob * sob).sum(dim=1).mean(dim=(1, 2))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "focus_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    torch_route.laplace = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], device=dev).reshape(1, 1, 3, 3)
    gx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], device=dev)
    torch_route.sobel = torch.stack([gx, gx.t()]).reshape(2, 1, 3, 3)

    def check(rc: int) -> None:
        if rc != 0:
            raise RuntimeError(_native.last_error())

    results = []
    for n, size, dtype in CONFIGS:
        images = real_batch(n, size, dtype).to(dev)
        code = _native.DTYPE_CODES[dtype]
        levels, scratch = (torch.empty((n, size, size), dtype=torch.uint8, device=dev) for _ in range(2))
        hist = torch.zeros((n, 256), dtype=torch.int64, device=dev)
        out = torch.empty((4 * n * (-(-size // 16)) ** 2,), dtype=torch.int64, device=dev)      # room for the finest grid
        tissue, counts = tissue_mask(images)
        check(lib.sx_grey_map(images.data_ptr(), code, n, size, size, 0, levels.data_ptr(), stream))
        torch.cuda.synchronize()

        def statistics(bh: int, bw: int, pooled: int = 0, masked: bool = False):
            if masked:
                return lambda: check(lib.sx_focus_statistics_masked(images.data_ptr(), code, n, size, size, 0, bh, bw, pooled, tissue.data_ptr(), out.data_ptr(), stream))
            return lambda: check(lib.sx_focus_statistics(images.data_ptr(), code, n, size, size, 0, bh, bw, pooled, out.data_ptr(), stream))

        forms = {"luminosity_histogram": lambda: check(lib.sx_luminosity_histogram(images.data_ptr(), code, n, size, size, 0, 0, hist.data_ptr(), stream)),
                 "saturation_map": lambda: check(lib.sx_saturation_map(images.data_ptr(), code, n, size, size, 0, scratch.data_ptr(), stream)),
                 "median_3": lambda: check(lib.sx_median_filter_u8(levels.data_ptr(), scratch.data_ptr(), n, size, size, 3, stream)),
                 "grey_map": lambda: check(lib.sx_grey_map(images.data_ptr(), code, n, size, size, 0, scratch.data_ptr(), stream)),
                 "focus_statistics_tile": statistics(0, 0),
                 "focus_statistics_64x64": statistics(64, 64),
                 "focus_statistics_16x16": statistics(16, 16),
                 "focus_statistics_tile_masked": statistics(0, 0, masked=True),
                 "focus_statistics_64x64_masked": statistics(64, 64, masked=True),
                 "focus_statistics_pooled": statistics(0, 0, pooled=1),
                 "focus_mask": lambda: focus_mask(images, MIN_VARIANCE, block=(64, 64)),
                 "focus_mask_given_tissue": lambda: focus_mask(images, MIN_VARIANCE, block=(64, 64), mask=tissue),
                 "torch_route": lambda: torch_route(images)}
        for fn in forms.values():      # warm-up
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls if form != "torch_route" else max(args.calls // 10, 5)))
        det = focus_mask(images, MIN_VARIANCE, block=(64, 64), mask=tissue)
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "calls_per_window": args.calls, "tissue_share": float(counts.sum().item()) / tissue.numel(),
               "min_variance": MIN_VARIANCE, "sharp_share_of_tissue": float(det.counts.sum().item()) / max(float(counts.sum().item()), 1.0)}
        yardstick = float(np.mean(times["luminosity_histogram"]))
        for form, values in times.items():
            mean = float(np.mean(values))
            row[form] = {"mean_us": mean, "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_luminosity_histogram": mean / yardstick,
                         "input_bytes_per_second": images.numel() * images.element_size() / (mean * 1e-6)}
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "library_bytes": _native.LIB_PATH.stat().st_size, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
