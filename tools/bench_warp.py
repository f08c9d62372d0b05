"""Cost of the affine warp through the C ABI -- sx_affine_warp with a row per tile -- on 64 x 3 x 512 x 512 uint8 and float32 batches cut
from the real-tissue fixture and a 256 x 3 x 224 x 224 bfloat16 batch, alternated in ONE process with
  sx_hsv_apply        the same bytes in and out, a streaming kernel: what a pass over the batch costs;
  sx_gaussian_blur    at sigma 1: the other kernel of the augmentation set that is not a stream;
  the torch route     element -> float32, affine_grid + grid_sample(padding_mode="reflection", align_corners=True), round (uint8), cast:
                      what a user has without this kernel (the normalised matrices are made once, outside the timed call);
and timed with device events over windows of back-to-back launches after a warm-up, medians of the windows.  The rows: a shift by a
quarter pixel (not the copy path); rotations by 10, 45 and 90 degrees, each with the quarter-pixel shift; a mixed draw per tile (rotation
over the full circle, scale 0.8 to 1.25); nearest, the constant border and -- uint8 only -- NHWC at 45 degrees; the 320 -> 224 crop at 45
degrees (its hsv / blur figures are those of the 224 output's bytes); the copy path (NaN rows).  The ratios are reported, not gated.  Each
case also records the largest difference between the kernel and the torch route (levels, or values of float tiles).
    python tools/bench_warp.py [--out profiles/warp_bench.json] [--calls 100] [--torch-calls 10] [--repeats 5]"""
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

from stainx_amd import HSVAugment, _native, affine_rows  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

NEAREST, BILINEAR = _native.WARP_INTERPOLATIONS["nearest"], _native.WARP_INTERPOLATIONS["bilinear"]
MIRROR, CONSTANT = _native.WARP_BORDERS["mirror"], _native.WARP_BORDERS["constant"]


def normalised(rows: torch.Tensor, h: int, w: int, oh: int, ow: int) -> torch.Tensor:
    """(N, 2, 3) matrices of affine_grid(align_corners=True) for pixel-index rows: x_n = 2 x / (W - 1) - 1 on both sides."""
    a, b, c, d, e, f = rows.double().unbind(1)
    top = torch.stack([a * (ow - 1) / (w - 1), b * (oh - 1) / (w - 1), (a * (ow - 1) + b * (oh - 1) + 2 * c) / (w - 1) - 1], 1)
    bottom = torch.stack([d * (ow - 1) / (h - 1), e * (oh - 1) / (h - 1), (d * (ow - 1) + e * (oh - 1) + 2 * f) / (h - 1) - 1], 1)
    return torch.stack([top, bottom], 1).float()


def torch_route(x: torch.Tensor, rows: torch.Tensor, oh: int, ow: int, nearest: bool, constant: bool):
    theta = normalised(rows, x.shape[2], x.shape[3], oh, ow)

    def run() -> torch.Tensor:
        grid = F.affine_grid(theta, (x.shape[0], 3, oh, ow), align_corners=True)
        y = F.grid_sample(x.to(torch.float32), grid, mode="nearest" if nearest else "bilinear", padding_mode="zeros" if constant else "reflection", align_corners=True)
        return torch.round(y).to(torch.uint8) if x.dtype == torch.uint8 else y.to(x.dtype)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "warp_bench.json"))
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
        sigmas = torch.ones(n, dtype=torch.float32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(2)
        quarter = (0.25, 0.25)
        cases = [("shift_0.25", x, size, affine_rows(n, (size, size), translate=quarter, device=dev), BILINEAR, MIRROR, False)]
        for angle in (10.0, 45.0, 90.0):
            cases.append((f"rotate_{angle:g}", x, size, affine_rows(n, (size, size), angle=angle, translate=quarter, device=dev), BILINEAR, MIRROR, False))
        mixed = affine_rows(n, (size, size), angle=torch.rand(n, generator=gen, device=dev) * 360.0 - 180.0, scale=0.8 + 0.45 * torch.rand(n, generator=gen, device=dev), device=dev)
        at_45 = affine_rows(n, (size, size), angle=45.0, translate=quarter, device=dev)
        cases += [("mixed", x, size, mixed, BILINEAR, MIRROR, False), ("nearest_45", x, size, at_45, NEAREST, MIRROR, False), ("constant_45", x, size, at_45, BILINEAR, CONSTANT, False)]
        if dtype == torch.uint8:
            cases.append(("nhwc_45", x.permute(0, 2, 3, 1).contiguous(), size, at_45, BILINEAR, MIRROR, True))
        cases.append(("crop_320_to_224_45", larger, 224, affine_rows(n, (320, 320), (224, 224), angle=45.0, translate=quarter, device=dev), BILINEAR, MIRROR, False))
        cases.append(("copy", x, size, torch.full((n, 6), float("nan"), device=dev), BILINEAR, MIRROR, False))
        for name, src, out_side, rows, interpolation, border, last in cases:
            rows = rows.contiguous()
            in_side = src.shape[1] if last else src.shape[2]
            out = torch.empty((n, out_side, out_side, 3) if last else (n, 3, out_side, out_side), dtype=dtype, device=dev)
            same = torch.empty((n, 3, out_side, out_side), dtype=dtype, device=dev)      # what the two streaming-sized siblings read and write: the output's bytes
            same_out = torch.empty_like(same)
            flags = _native.MACENKO_CHANNELS_LAST if last else 0
            planar = src.permute(0, 3, 1, 2).contiguous() if last else src
            forms = {"hsv_apply": (lambda: check(lib.sx_hsv_apply(same.data_ptr(), same_out.data_ptr(), code, n, out_side, out_side, hsv_rows.data_ptr(), n, 0, stream)), args.calls),
                     "gaussian_blur": (lambda: check(lib.sx_gaussian_blur(same.data_ptr(), same_out.data_ptr(), code, n, out_side, out_side, sigmas.data_ptr(), n, 0, stream)), args.calls),
                     "affine_warp": (lambda: check(lib.sx_affine_warp(src.data_ptr(), out.data_ptr(), code, n, in_side, in_side, out_side, out_side, rows.data_ptr(), n, interpolation, border, 0.0,
                                                                      flags, stream)), args.calls)}
            if name != "copy":
                forms["torch_route"] = (torch_route(planar, rows, out_side, out_side, interpolation == NEAREST, border == CONSTANT), args.torch_calls)
            same.copy_(planar[:, :, :out_side, :out_side])
            for fn, _ in forms.values():      # warm-up
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {form: [] for form in forms}
            for _ in range(args.repeats):      # alternated: one window of each form per repeat
                for form, (fn, calls) in forms.items():
                    times[form].append(window(fn, calls))
            bytes_moved = (src.numel() + out.numel()) * x.element_size()
            row = {"dtype": str(dtype).replace("torch.", ""), "source": list(src.shape), "output": list(out.shape), "rows": name, "windows": args.repeats,
                   "bytes_of_source_and_output": bytes_moved}
            for form, values in times.items():
                row[form] = {"calls_per_window": forms[form][1], "median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            row["warp_to_hsv_apply"] = row["affine_warp"]["median_us"] / row["hsv_apply"]["median_us"]
            row["warp_to_gaussian_blur"] = row["affine_warp"]["median_us"] / row["gaussian_blur"]["median_us"]
            if "torch_route" in forms:
                row["torch_route_to_warp"] = row["torch_route"]["median_us"] / row["affine_warp"]["median_us"]
                got = out.permute(0, 3, 1, 2) if last else out
                row["max_abs_diff_to_torch_route"] = float((got.double() - forms["torch_route"][0]().double()).abs().max())
            results.append(row)
            print(json.dumps(row))
    size_mb = {path.name: round(path.stat().st_size / 1e6, 2) for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH) if path.exists()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "library_mb": size_mb, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
