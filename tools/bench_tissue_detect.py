"""Cost of tissue detection: the luminosity histogram, the rule with a cut per tile and each morphology op through the C ABI on a batch cut
from the real-tissue fixture, alternated with sx_tissue_mask in ONE process, timed with device events.
    python tools/bench_tissue_detect.py [--out profiles/tissue_detect_bench.json] [--calls 200] [--repeats 3]
Every figure is compared with sx_tissue_mask OF THE SAME RUN; the spread of the repeats is reported with the means."""
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

RADII = (2, 5, 15)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tissue_detect_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    n, size = args.tiles, args.size
    results = []
    for dtype in (torch.uint8, torch.float32):
        x = real_batch(n, size, dtype).to(dev)
        code, stream = _native.DTYPE_CODES[dtype], _native.stream_ptr(dev)
        mask = torch.empty((n, size, size), dtype=torch.uint8, device=dev)
        out, scratch = torch.empty_like(mask), torch.empty_like(mask)
        counts = torch.zeros((n,), dtype=torch.int64, device=dev)
        hist = torch.zeros((n, 256), dtype=torch.int64, device=dev)
        cuts = torch.full((n,), lib.sx_tissue_y_cut(0.8), dtype=torch.float32, device=dev)

        def check(rc: int) -> None:
            if rc != 0:
                raise RuntimeError(_native.last_error())

        forms = {"tissue_mask": lambda: check(lib.sx_tissue_mask(x.data_ptr(), code, n, size, size, 0, 0.8, mask.data_ptr(), counts.data_ptr(), stream)),
                 "tissue_mask_tiles": lambda: check(lib.sx_tissue_mask_tiles(x.data_ptr(), code, n, size, size, 0, cuts.data_ptr(), mask.data_ptr(), counts.data_ptr(), stream)),
                 "luminosity_histogram": lambda: check(lib.sx_luminosity_histogram(x.data_ptr(), code, n, size, size, 0, 0, hist.data_ptr(), stream)),
                 "luminosity_histogram_pooled": lambda: check(lib.sx_luminosity_histogram(x.data_ptr(), code, n, size, size, 0, 1, hist.data_ptr(), stream))}
        for element in _native.MORPH_ELEMENTS:
            for op in _native.MORPH_OPS:
                for radius in RADII:
                    forms[f"{op}_{element}_r{radius}"] = (lambda op=op, element=element, radius=radius: check(lib.sx_mask_morphology(
                        mask.data_ptr(), out.data_ptr(), n, size, size, _native.MORPH_OPS[op], _native.MORPH_ELEMENTS[element], radius, scratch.data_ptr(), counts.data_ptr(), stream)))
        forms["tissue_mask"]()      # (the morphology forms read this mask)
        for fn in forms.values():      # warm-up
            for _ in range(10):
                fn()
        forms["tissue_mask"]()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for name, fn in forms.items():
                times[name].append(window(fn, args.calls))
            forms["tissue_mask"]()
        row = {"shape": [n, 3, size, size], "dtype": str(dtype).replace("torch.", ""), "tissue_share": float(mask.sum().item()) / mask.numel(), "calls_per_window": args.calls}
        base = float(np.mean(times["tissue_mask"]))
        for name, values in times.items():
            row[name] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_tissue_mask": float(np.mean(values)) / base}
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
