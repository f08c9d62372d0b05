"""Cost of the tone jitter and of the grey statistics through the C ABI, on 64 x 3 x 512 x 512 uint8 and float32 batches cut from the
real-tissue fixture and a 256 x 3 x 224 x 224 bfloat16 batch.  Every form is alternated in ONE process with sx_hsv_apply on the same bytes
(the same read, the same write) and timed with device events over windows of back-to-back launches after a warm-up:
  sx_tone_apply without seeds (brightness / contrast / gamma rows), with noise per channel and with shared noise, against sx_hsv_apply;
  the torch route for both forms: x * a + b, (+ randn_like * sigma), clamp, round and the cast, with float temporaries;
  sx_grey_statistics per tile, pooled and masked, against sx_grey_map + sx_level_histogram (two launches and a one-byte map).
Ratios are reported, not gated.  NCHW only: the NHWC forms and the masked tone jitter are not timed here.
    python tools/bench_tone.py [--out profiles/tone_bench.json] [--calls 100] [--repeats 5]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import HSVAugment, ToneAugment, _native  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tone_bench.json"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _native.require()
    stream = _native.stream_ptr(dev)
    results = []
    for n, size, dtype in ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16)):
        code = _native.DTYPE_CODES[dtype]
        x = real_batch(n, size, dtype).to(dev)
        out = torch.empty_like(x)
        gen = torch.Generator(device=dev).manual_seed(1)
        hsv_rows = HSVAugment(0.05, 0.1, 0.1, saturation_shift=0.02, value_shift=0.02, generator=gen).sample_rows(n, dev).contiguous()
        aug = ToneAugment(0.2, 0.2, gamma=0.0, noise=0.05, pivot=0.5, generator=gen)
        rows = aug.sample_rows(n, None, dev).contiguous()
        curved = rows.clone()
        curved[:, 2] = torch.exp(0.3 * (2.0 * torch.rand(n, generator=gen, device=dev) - 1.0))
        seeds = aug.sample_seeds(n, dev).contiguous()
        mask = (torch.rand((n, size, size), generator=gen, device=dev) < 0.6).to(torch.uint8)
        grey = torch.empty((n, size, size), dtype=torch.uint8, device=dev)
        hist = torch.empty((n, 256), dtype=torch.int64, device=dev)
        words = torch.empty((n, 3), dtype=torch.int64, device=dev)
        a, b, sigma = (rows[:, k].reshape(n, 1, 1, 1).contiguous() for k in (0, 1, 3))
        scale = 255.0 if dtype == torch.uint8 else 1.0

        def check(rc: int) -> None:
            assert rc == 0, _native.last_error()

        def torch_route(noise: bool) -> None:
            t = x.to(torch.float32) * a + b * scale
            if noise:
                t = t + torch.randn_like(t) * (sigma * scale)
            t = t.clamp(0.0, scale)
            out.copy_(t.round() if dtype == torch.uint8 else t)

        def grey_two_launches() -> None:
            check(lib.sx_grey_map(x.data_ptr(), code, n, size, size, 0, grey.data_ptr(), stream))
            check(lib.sx_level_histogram(grey.data_ptr(), n, size, size, 0, hist.data_ptr(), stream))

        def tone(r: torch.Tensor, s, shared: int):
            return lambda: check(lib.sx_tone_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, r.data_ptr(), n, s, shared, 0, stream))

        forms = {"hsv_apply": lambda: check(lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, hsv_rows.data_ptr(), n, 0, stream)),
                 "tone_apply": tone(rows, None, 0),
                 "tone_apply_gamma": tone(curved, None, 0),
                 "tone_apply_noise": tone(rows, seeds.data_ptr(), 0),
                 "tone_apply_shared_noise": tone(rows, seeds.data_ptr(), 1),
                 "torch_affine": lambda: torch_route(False),
                 "torch_affine_noise": lambda: torch_route(True),
                 "grey_map_level_histogram": grey_two_launches,
                 "grey_statistics": lambda: check(lib.sx_grey_statistics(x.data_ptr(), code, n, size, size, 0, 0, words.data_ptr(), stream)),
                 "grey_statistics_pooled": lambda: check(lib.sx_grey_statistics(x.data_ptr(), code, n, size, size, 0, 1, words.data_ptr(), stream)),
                 "grey_statistics_masked": lambda: check(lib.sx_grey_statistics_masked(x.data_ptr(), code, n, size, size, 0, 0, mask.data_ptr(), words.data_ptr(), stream))}
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
        for form in ("tone_apply", "tone_apply_gamma", "tone_apply_noise", "tone_apply_shared_noise"):
            row[form]["gb_per_s_at_median"] = bytes_moved / row[form]["median_us"] / 1e3
            row[form + "_to_hsv_apply"] = row[form]["median_us"] / row["hsv_apply"]["median_us"]
        row["torch_affine_to_tone_apply"] = row["torch_affine"]["median_us"] / row["tone_apply"]["median_us"]
        row["torch_affine_noise_to_tone_apply_noise"] = row["torch_affine_noise"]["median_us"] / row["tone_apply_noise"]["median_us"]
        for form in ("grey_statistics", "grey_statistics_pooled", "grey_statistics_masked"):
            row[form + "_to_grey_map_level_histogram"] = row[form]["median_us"] / row["grey_map_level_histogram"]["median_us"]
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
