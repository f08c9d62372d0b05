"""Cost of the JPEG round trip through the C ABI, on 64 x 3 x 512 x 512 uint8 and float32 batches cut from the real-tissue fixture and a
256 x 3 x 224 x 224 bfloat16 batch.  Every form is alternated in ONE process with sx_hsv_apply on the same bytes (the same read, the same
write: the streaming yardstick) and with sx_gaussian_blur at sigma 1 (the other kernel that keeps a block on chip), and timed with device
events over windows of back-to-back launches after a warm-up:
  sx_jpeg_roundtrip at quality 30, 75, 95 and a mixed row (a quality per tile drawn from 30..95), at 4:4:4 and 4:2:0.
Where Pillow is installed the CPU route is a separate figure on the uint8 batch: the batch copied to the host, every tile saved and opened
again by at most 16 threads, the result copied back -- wall time, copies included, NOT a device-event time.
Ratios are reported, not gated.  NCHW only: NHWC, the masked call, float16 / float64 and ``JPEGAugment.forward`` are not timed here.
    python tools/bench_jpeg.py [--out profiles/jpeg_bench.json] [--calls 50] [--repeats 5]"""
from __future__ import annotations

import argparse
import io
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import HSVAugment, JPEGAugment, _native  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

QUALITIES = (30, 75, 95)


def pillow_route(x: torch.Tensor, qualities: np.ndarray, subsampling: int, pool: ThreadPoolExecutor) -> float:
    """Seconds of one batch through Pillow: device -> host, save / open per tile, host -> device."""
    from PIL import Image

    def one(job):
        hwc, q = job
        buffer = io.BytesIO()
        Image.fromarray(hwc, "RGB").save(buffer, "JPEG", quality=int(q), subsampling=subsampling)
        buffer.seek(0)
        return np.asarray(Image.open(buffer).convert("RGB"))

    torch.cuda.synchronize()
    start = time.perf_counter()
    host = x.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    done = np.stack(list(pool.map(one, zip(host, qualities))))
    back = torch.from_numpy(done).to(x.device).permute(0, 3, 1, 2).contiguous()
    torch.cuda.synchronize()
    assert back.shape == x.shape
    return time.perf_counter() - start


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jpeg_bench.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    results = []
    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        code = _native.DTYPE_CODES[dtype]
        x = real_batch(n, size, dtype).to(dev)
        out = torch.empty_like(x)
        gen = torch.Generator(device=dev).manual_seed(1)
        hsv_rows = HSVAugment(0.05, 0.1, 0.1, saturation_shift=0.02, value_shift=0.02, generator=gen).sample_rows(n, dev).contiguous()
        sigmas = torch.ones(n, dtype=torch.float32, device=dev)
        rows = {f"q{q}": torch.full((n,), float(q), dtype=torch.float32, device=dev) for q in QUALITIES}
        rows["mixed"] = JPEGAugment((30, 95), generator=gen).sample_rows(n, dev).contiguous()

        def check(rc: int) -> None:
            assert rc == 0, _native.last_error()

        def jpeg(r: torch.Tensor, sub: int):
            return lambda: check(lib.sx_jpeg_roundtrip(x.data_ptr(), out.data_ptr(), code, n, size, size, r.data_ptr(), n, sub, 0, stream))

        forms = {"hsv_apply": lambda: check(lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, hsv_rows.data_ptr(), n, 0, stream)),
                 "gaussian_blur_sigma1": lambda: check(lib.sx_gaussian_blur(x.data_ptr(), out.data_ptr(), code, n, size, size, sigmas.data_ptr(), n, 0, stream))}
        for sub, name in ((0, "444"), (2, "420")):
            for key, r in rows.items():
                forms[f"jpeg_{name}_{key}"] = jpeg(r, sub)
        for fn in forms.values():      # warm-up
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        bytes_moved = 2 * x.numel() * x.element_size()
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "calls_per_window": args.calls, "windows": args.repeats, "bytes_read_and_written": bytes_moved}
        for form, values in times.items():
            row[form] = {"median_us": float(np.median(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
        for form in forms:
            if form.startswith("jpeg_"):
                row[form]["gb_per_s_at_median"] = bytes_moved / row[form]["median_us"] / 1e3
                row[form + "_to_hsv_apply"] = row[form]["median_us"] / row["hsv_apply"]["median_us"]
                row[form + "_to_gaussian_blur"] = row[form]["median_us"] / row["gaussian_blur_sigma1"]["median_us"]
        if pillow is not None and dtype == torch.uint8:      # the CPU route: wall time, copies included
            qualities = rows["mixed"].cpu().numpy()
            with ThreadPoolExecutor(max_workers=16) as pool:
                for sub, name in ((0, "444"), (2, "420")):
                    pillow_route(x, qualities, sub, pool)      # warm-up
                    walls = [pillow_route(x, qualities, sub, pool) for _ in range(3)]
                    row[f"pillow_{name}_mixed_wall"] = {"median_us": float(np.median(walls)) * 1e6, "min_us": float(np.min(walls)) * 1e6, "max_us": float(np.max(walls)) * 1e6, "threads": 16,
                                                        "pillow": pillow}
                    row[f"pillow_{name}_mixed_wall_to_jpeg"] = row[f"pillow_{name}_mixed_wall"]["median_us"] / row[f"jpeg_{name}_mixed"]["median_us"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "pillow": pillow, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
