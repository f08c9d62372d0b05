"""Cost of the elastic warp through the C ABI -- sx_elastic_warp with a row and a control grid per tile -- on 64 x 3 x 512 x 512 uint8 and
float32 batches cut from the real-tissue fixture and a 256 x 3 x 224 x 224 bfloat16 batch, alternated in ONE process with
  sx_affine_warp      the same mixed rows (rotation over the full circle, scale 0.8 to 1.25) without the grid: THE YARDSTICK -- what the
                      displacement adds to the gather;
  sx_hsv_apply        the output's bytes in and out, a streaming kernel: what a pass over the batch costs;
  the torch route     a dense flow from F.interpolate(grids, mode="bicubic") added to affine_grid, then grid_sample(padding_mode=
                      "reflection", align_corners=True), round (uint8), cast: what a user has without this kernel (the normalised matrices are
                      made once, outside the timed call; the bicubic flow is not the B-spline's, it costs what a dense flow costs);
and timed with device events over windows of back-to-back launches after a warm-up, medians of the windows (tools/bench_warp.py's method).
The settings: cells 8, 16 and 64 with control displacements of standard deviation 2 pixels; the zero grid at cell 16; the 320 -> 224 crop
at cell 16.  The ratios are reported, not gated.
    python tools/bench_elastic.py [--out profiles/elastic_bench.json] [--calls 100] [--torch-calls 10] [--repeats 5]"""
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

from stainx_amd import HSVAugment, _native, affine_rows, elastic_grids  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402
from tools.bench_warp import normalised  # noqa: E402

BILINEAR, MIRROR = _native.WARP_INTERPOLATIONS["bilinear"], _native.WARP_BORDERS["mirror"]


def torch_route(x: torch.Tensor, rows: torch.Tensor, grids: torch.Tensor, oh: int, ow: int):
    h, w = x.shape[2], x.shape[3]
    theta = normalised(rows, h, w, oh, ow)
    to_unit = torch.tensor([2.0 / (w - 1), 2.0 / (h - 1)], dtype=torch.float32, device=x.device)

    def run() -> torch.Tensor:
        flow = F.interpolate(grids, size=(oh, ow), mode="bicubic", align_corners=False)      # (N, 2, OH, OW): the dense field
        grid = F.affine_grid(theta, (x.shape[0], 3, oh, ow), align_corners=True) + flow.permute(0, 2, 3, 1) * to_unit
        y = F.grid_sample(x.to(torch.float32), grid, mode="bilinear", padding_mode="reflection", align_corners=True)
        return torch.round(y).to(torch.uint8) if x.dtype == torch.uint8 else y.to(x.dtype)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "elastic_bench.json"))
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
        larger = real_batch(n, 320, dtype).to(dev)      # the source of the 320 -> 224 crop
        hsv_rows = HSVAugment(0.05, 0.1, 0.1, generator=torch.Generator(device=dev).manual_seed(1)).sample_rows(n, dev).contiguous()
        gen = torch.Generator(device=dev).manual_seed(2)
        angle, scale = torch.rand(n, generator=gen, device=dev) * 360.0 - 180.0, 0.8 + 0.45 * torch.rand(n, generator=gen, device=dev)
        mixed = affine_rows(n, (size, size), angle=angle, scale=scale, device=dev).contiguous()
        cropping = affine_rows(n, (320, 320), (224, 224), angle=angle, scale=scale, device=dev).contiguous()
        cases = [(f"cell_{cell}", x, size, mixed, cell, 2.0) for cell in (8, 16, 64)]
        cases += [("zero_grid_cell_16", x, size, mixed, 16, 0.0), ("crop_320_to_224_cell_16", larger, 224, cropping, 16, 2.0)]
        for name, src, out_side, rows, cell, magnitude in cases:
            in_side = src.shape[2]
            grids = elastic_grids(n, (out_side, out_side), cell, magnitude, generator=gen, device=dev).contiguous()
            out = torch.empty((n, 3, out_side, out_side), dtype=dtype, device=dev)
            same = torch.empty((n, 3, out_side, out_side), dtype=dtype, device=dev)      # what the streaming sibling reads and writes: the output's bytes
            same_out = torch.empty_like(same)
            same.copy_(src[:, :, :out_side, :out_side])
            forms = {"hsv_apply": (lambda: check(lib.sx_hsv_apply(same.data_ptr(), same_out.data_ptr(), code, n, out_side, out_side, hsv_rows.data_ptr(), n, 0, stream)), args.calls),
                     "affine_warp": (lambda: check(lib.sx_affine_warp(src.data_ptr(), out.data_ptr(), code, n, in_side, in_side, out_side, out_side, rows.data_ptr(), n, BILINEAR, MIRROR, 0.0, 0,
                                                                      stream)), args.calls),
                     "elastic_warp": (lambda: check(lib.sx_elastic_warp(src.data_ptr(), out.data_ptr(), code, n, in_side, in_side, out_side, out_side, rows.data_ptr(), n, grids.data_ptr(), n, cell,
                                                                        BILINEAR, MIRROR, 0.0, 0, stream)), args.calls),
                     "torch_route": (torch_route(src, rows, grids, out_side, out_side), args.torch_calls)}
            for fn, _ in forms.values():      # warm-up
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {form: [] for form in forms}
            for _ in range(args.repeats):      # alternated: one window of each form per repeat
                for form, (fn, calls) in forms.items():
                    times[form].append(window(fn, calls))
            row = {"dtype": str(dtype).replace("torch.", ""), "source": list(src.shape), "output": list(out.shape), "setting": name, "cell": cell, "magnitude": magnitude,
                   "grid_bytes": grids.numel() * 4, "windows": args.repeats, "bytes_of_source_and_output": (src.numel() + out.numel()) * x.element_size()}
            for form, values in times.items():
                row[form] = {"calls_per_window": forms[form][1], "median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            row["elastic_to_affine_warp"] = row["elastic_warp"]["median_us"] / row["affine_warp"]["median_us"]
            row["elastic_to_hsv_apply"] = row["elastic_warp"]["median_us"] / row["hsv_apply"]["median_us"]
            row["torch_route_to_elastic"] = row["torch_route"]["median_us"] / row["elastic_warp"]["median_us"]
            results.append(row)
            print(json.dumps(row))
    size_mb = {path.name: round(path.stat().st_size / 1e6, 2) for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH) if path.exists()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "library_mb": size_mb, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
