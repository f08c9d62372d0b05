"""Cost of the Vahadane estimate (sx_vahadane_estimate at 10 and 30 rounds, with and without the percentiles), of the percentile call
(sx_stain_max_concentrations) and of Vahadane.transform on 64 x 3 x 512 x 512 uint8 and float32 and 256 x 3 x 224 x 224 bfloat16 batches cut
from the real-tissue fixture, alternated in ONE process with sx_macenko_estimate and Macenko.transform and timed with device events.
    python tools/bench_vahadane.py [--out profiles/vahadane_bench.json] [--calls 20] [--repeats 3]
The calls go through the backend engines (the output tensors of a call come from torch's caching allocator; the batches keep the GPU busy
for hundreds of microseconds per call).  Every figure is also a ratio to sx_macenko_estimate / Macenko.transform OF THE SAME RUN.  The time
per round is (t30 - t10) / 20 of the estimate without percentiles; with it the bytes of the images one round reads per second, to be held
against the HBM's peak (rounds after the first can be served by the Infinity Cache), and the pixels per second, to be compared between
uint8 tiles (optical densities from a table) and float tiles (three logarithms per pixel and round)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import Macenko, Vahadane, stain_basis  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

WORKLOADS = ((64, 512, torch.uint8), (64, 512, torch.float32), (256, 224, torch.bfloat16))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vahadane_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    init = stain_basis("he")[:, :2].to(dev)
    results = []
    for n, size, dtype in WORKLOADS:
        images = real_batch(n, size, dtype).to(dev)
        reference = images[:1]
        macenko = Macenko(device=dev).fit(reference)
        vahadane = Vahadane(device=dev, mask=None).fit(reference)            # every pixel: the same pixels as the Macenko calls
        masked = Vahadane(device=dev).fit(reference)                         # the default: over the luminosity mask, glass copied
        m_engine, v_engine = macenko._get_backend_impl(), vahadane._get_backend_impl()
        he = vahadane.estimate(images).stain_matrices
        forms = {"macenko_estimate": lambda: m_engine.estimate(images),
                 "macenko_transform": lambda: macenko.transform(images),
                 "vahadane_estimate_10_no_maxc": lambda: v_engine.vahadane_estimate(images, init, iterations=10, max_conc=False),
                 "vahadane_estimate_30_no_maxc": lambda: v_engine.vahadane_estimate(images, init, iterations=30, max_conc=False),
                 "vahadane_estimate_10": lambda: v_engine.vahadane_estimate(images, init, iterations=10),
                 "vahadane_estimate_30": lambda: v_engine.vahadane_estimate(images, init, iterations=30),
                 "max_concentrations": lambda: v_engine.max_concentrations(images, he),
                 "vahadane_transform": lambda: vahadane.transform(images),
                 "vahadane_transform_luminosity_mask": lambda: masked.transform(images)}
        for fn in forms.values():      # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {form: [] for form in forms}
        for _ in range(args.repeats):      # alternated: one window of each form per repeat
            for form, fn in forms.items():
                times[form].append(window(fn, args.calls))
        row = {"dtype": str(dtype).replace("torch.", ""), "shape": [n, 3, size, size], "calls_per_window": args.calls, "regularizer": 0.1}
        estimate, transform = float(np.mean(times["macenko_estimate"])), float(np.mean(times["macenko_transform"]))
        for form, values in times.items():
            mean = float(np.mean(values))
            row[form] = {"mean_us": mean, "min_us": float(np.min(values)), "max_us": float(np.max(values)),
                         "ratio_to_macenko_transform" if "transform" in form else "ratio_to_macenko_estimate": mean / (transform if "transform" in form else estimate)}
        per_round = (row["vahadane_estimate_30_no_maxc"]["mean_us"] - row["vahadane_estimate_10_no_maxc"]["mean_us"]) / 20.0
        row["round_us"] = per_round
        row["round_image_bytes_per_second"] = images.numel() * images.element_size() / (per_round * 1e-6)
        row["round_pixels_per_second"] = n * size * size / (per_round * 1e-6)
        results.append(row)
        print(json.dumps(row))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
