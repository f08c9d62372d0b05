"""Cost of saturation-channel tissue detection through the C ABI: sx_saturation_map, sx_median_filter_u8 (sizes 3, 7 and 15),
sx_level_histogram (per tile and pooled) and sx_level_mask_tiles on 64 x 512 x 512 uint8 and float32 batches cut from the real-tissue
fixture, alternated in ONE process with sx_tissue_mask and with an sx_mask_morphology opening (disk, r = 2), timed with device events.
    python tools/bench_saturation.py [--out profiles/saturation_bench.json] [--calls 200] [--repeats 3]
Every figure is compared with sx_tissue_mask and with the opening OF THE SAME RUN; the spread of the repeats is reported with the means.
The median rows also carry the useful work -- the levels of every window, size^2 per output pixel -- per second."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

MEDIAN_SIZES = (3, 7, 15)
THRESHOLD = 8


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "saturation_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    n, size = args.tiles, args.size
    stream = _native.stream_ptr(dev)
    levels, filtered, made, opened, scratch = (torch.empty((n, size, size), dtype=torch.uint8, device=dev) for _ in range(5))
    counts = torch.zeros((n,), dtype=torch.int64, device=dev)
    hist = torch.zeros((n, 256), dtype=torch.int64, device=dev)
    cuts = torch.full((n,), THRESHOLD, dtype=torch.int32, device=dev)

    def check(rc: int) -> None:
        if rc != 0:
            raise RuntimeError(_native.last_error())

    results = []
    for dtype in (torch.uint8, torch.float32):
        images = real_batch(n, size, dtype).to(dev)
        code = _native.DTYPE_CODES[dtype]
        # the inputs of the later steps: the saturation map of this batch, its 7 x 7 median, the mask at CLAM's level
        check(lib.sx_saturation_map(images.data_ptr(), code, n, size, size, 0, levels.data_ptr(), stream))
        check(lib.sx_median_filter_u8(levels.data_ptr(), filtered.data_ptr(), n, size, size, 7, stream))
        check(lib.sx_level_mask_tiles(filtered.data_ptr(), n, size, size, cuts.data_ptr(), made.data_ptr(), counts.data_ptr(), stream))
        torch.cuda.synchronize()
        set_share = float(counts.sum().item()) / made.numel()
        forms = {"tissue_mask": lambda: check(lib.sx_tissue_mask(images.data_ptr(), code, n, size, size, 0, 0.8, opened.data_ptr(), counts.data_ptr(), stream)),
                 "open_disk_r2": lambda: check(lib.sx_mask_morphology(made.data_ptr(), opened.data_ptr(), n, size, size, _native.MORPH_OPS["open"], _native.MORPH_ELEMENTS["disk"], 2,
                                                                      scratch.data_ptr(), counts.data_ptr(), stream)),
                 "saturation_map": lambda: check(lib.sx_saturation_map(images.data_ptr(), code, n, size, size, 0, scratch.data_ptr(), stream))}
        for k in MEDIAN_SIZES:
            forms[f"median_{k}"] = lambda k=k: check(lib.sx_median_filter_u8(levels.data_ptr(), scratch.data_ptr(), n, size, size, k, stream))
        forms["level_histogram"] = lambda: check(lib.sx_level_histogram(filtered.data_ptr(), n, size, size, 0, hist.data_ptr(), stream))
        forms["level_histogram_pooled"] = lambda: check(lib.sx_level_histogram(filtered.data_ptr(), n, size, size, 1, hist.data_ptr(), stream))
        forms["level_mask_tiles"] = lambda: check(lib.sx_level_mask_tiles(filtered.data_ptr(), n, size, size, cuts.data_ptr(), opened.data_ptr(), counts.data_ptr(), stream))
        for fn in forms.values():      # warm-up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, size, size], "threshold": THRESHOLD, "set_share_at_threshold": set_share, "calls_per_window": args.calls}
        rule, opening = float(np.mean(times["tissue_mask"])), float(np.mean(times["open_disk_r2"]))
        for form, values in times.items():
            mean = float(np.mean(values))
            row[form] = {"mean_us": mean, "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_tissue_mask": mean / rule, "ratio_to_open_disk_r2": mean / opening}
            if form.startswith("median_"):
                k = int(form.split("_")[1])
                row[form]["window_levels_per_second"] = n * size * size * k * k / (mean * 1e-6)
                row[form]["output_pixels_per_second"] = n * size * size / (mean * 1e-6)
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
