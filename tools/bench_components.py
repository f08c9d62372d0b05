"""Cost of the mask components: sx_mask_components and sx_mask_area_filter (objects and holes, connectivity 4 and 8) through the C ABI on
64 x 512 x 512 masks -- the Otsu masks of a batch cut from the real-tissue fixture, an all-set batch (every pixel one component: the
contention case) and a random batch at density 0.5 -- alternated in ONE process with the step the filter replaces, an sx_mask_morphology
opening of radius 2, and with sx_tissue_mask, timed with device events.
    python tools/bench_components.py [--out profiles/components_bench.json] [--calls 200] [--repeats 3]
Every figure is compared with the opening and with sx_tissue_mask OF THE SAME RUN; the spread of the repeats is reported with the means."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import _native, otsu_mask  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

MIN_AREA = 64


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "components_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    n, size = args.tiles, args.size
    images = real_batch(n, size, torch.uint8).to(dev)
    u8, stream = _native.DTYPE_CODES[torch.uint8], _native.stream_ptr(dev)
    inputs = {"real_otsu": otsu_mask(images).mask,
              "all_set": torch.ones((n, size, size), dtype=torch.uint8, device=dev),
              "random_0.5": (torch.rand((n, size, size), device=dev, generator=torch.Generator(dev).manual_seed(7)) < 0.5).to(torch.uint8)}
    out, scratch, made = (torch.empty((n, size, size), dtype=torch.uint8, device=dev) for _ in range(3))
    labels, areas = (torch.empty((n, size, size), dtype=torch.int32, device=dev) for _ in range(2))
    counts = torch.zeros((n,), dtype=torch.int64, device=dev)
    workspace = torch.empty((int(lib.sx_mask_components_workspace_bytes(n, size, size)),), dtype=torch.uint8, device=dev)

    def check(rc: int) -> None:
        if rc != 0:
            raise RuntimeError(_native.last_error())

    results = []
    for name, mask in inputs.items():
        forms = {"tissue_mask": lambda: check(lib.sx_tissue_mask(images.data_ptr(), u8, n, size, size, 0, 0.8, made.data_ptr(), counts.data_ptr(), stream)),
                 "open_disk_r2": lambda: check(lib.sx_mask_morphology(mask.data_ptr(), out.data_ptr(), n, size, size, _native.MORPH_OPS["open"], _native.MORPH_ELEMENTS["disk"], 2,
                                                                      scratch.data_ptr(), counts.data_ptr(), stream))}
        for connectivity in _native.CONNECTIVITIES:
            forms[f"components_c{connectivity}"] = (lambda connectivity=connectivity: check(lib.sx_mask_components(
                mask.data_ptr(), n, size, size, connectivity, 0, labels.data_ptr(), areas.data_ptr(), counts.data_ptr(), stream)))
            for holes, what in ((0, "objects"), (1, "holes")):
                forms[f"remove_small_{what}_c{connectivity}"] = (lambda connectivity=connectivity, holes=holes: check(lib.sx_mask_area_filter(
                    mask.data_ptr(), out.data_ptr(), n, size, size, connectivity, holes, MIN_AREA, workspace.data_ptr(), counts.data_ptr(), stream)))
        for fn in forms.values():      # warm-up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        check(lib.sx_mask_components(mask.data_ptr(), n, size, size, 8, 0, labels.data_ptr(), areas.data_ptr(), counts.data_ptr(), stream))
        row = {"input": name, "shape": [n, size, size], "set_share": float(mask.sum().item()) / mask.numel(), "components_per_tile_c8": float(counts.sum().item()) / n,
               "min_area": MIN_AREA, "calls_per_window": args.calls}
        opening, rule = float(np.mean(times["open_disk_r2"])), float(np.mean(times["tissue_mask"]))
        for form, values in times.items():
            row[form] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values)), "ratio_to_open_disk_r2": float(np.mean(values)) / opening,
                         "ratio_to_tissue_mask": float(np.mean(values)) / rule}
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
