"""Cost of luminosity standardisation through the C ABI -- sx_luminosity_percentile (per tile and pooled) and sx_luminosity_apply -- and of
LuminosityStandardizer.forward on 64 x 3 x 512 x 512 uint8 and float32 batches: one cut from the real-tissue fixture, one "glass" batch in
which 92 % of the pixels are ONE value (the fixture's tissue only in a 144 x 144 corner of every tile).  Every call is alternated in ONE
process with the parent's calls and timed with device events, three windows each:
    sx_luminosity_percentile   against sx_stain_max_concentrations (the exact three-pass selection of two keys and three logarithms a pixel)
    sx_luminosity_percentile   on the glass batch against the tissue batch, and against the diagnostic build's form without the run
                               counting (one LDS add per pixel: sx_luminosity_percentile_plain)
    sx_luminosity_apply        against sx_reinhard_apply_stats (the one-launch LAB apply)
    forward                    against Reinhard(statistics="tile").transform
    python tools/bench_luminosity.py [--out profiles/luminosity_bench.json] [--calls 200] [--repeats 3]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from stainx_amd import LuminosityStandardizer, Reinhard, _native, stain_basis  # noqa: E402
from tools.bench_masked import real_batch, window  # noqa: E402

GLASS = (243, 241, 244)
CORNER = 144      # 144 x 144 of 512 x 512: 7.9 % tissue


def glass_batch(tissue_u8: torch.Tensor) -> torch.Tensor:
    out = torch.tensor(GLASS, dtype=torch.uint8).view(1, 3, 1, 1).expand_as(tissue_u8).clone()
    out[:, :, :CORNER, :CORNER] = tissue_u8[:, :, :CORNER, :CORNER]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "luminosity_bench.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, diag = _native.require(), _native.require_diag()
    stream = _native.stream_ptr(dev)
    n, size = 64, 512
    tissue_u8 = real_batch(n, size, torch.uint8)
    batches = {"tissue": tissue_u8, "glass": glass_batch(tissue_u8)}
    he = stain_basis("he")[:, :2].contiguous().to(dev)
    std = LuminosityStandardizer(95.0)
    results = []
    for dtype in (torch.uint8, torch.float32):
        code = _native.DTYPE_CODES[dtype]
        for kind, tiles in batches.items():
            from stainx_amd import synth

            x = synth.as_dtype(tiles, dtype).to(dev)
            out = torch.empty_like(x)
            lum, pixels = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
            max_c = torch.empty(n, 2, dtype=torch.float32, device=dev)
            ws = torch.empty(max(lib.sx_luminosity_workspace_bytes(code, n, size, size), lib.sx_vahadane_workspace_bytes(code, n, size, size)), dtype=torch.uint8, device=dev)
            reinhard = Reinhard(device=dev, statistics="tile").fit(x[:1])
            stats = reinhard.estimate(x)
            src_mean, src_std = stats.mean.contiguous(), stats.std.contiguous()
            ref_mean, ref_std = reinhard._reference_mean.to(dev).float().contiguous(), reinhard._reference_std.to(dev).float().contiguous()

            def check(rc: int) -> None:
                assert rc == 0, _native.last_error()

            def percentile(which, pooled: int):
                return lambda: check(which(x.data_ptr(), code, n, size, size, None, pooled, 95.0, lum.data_ptr(), pixels.data_ptr(), ws.data_ptr(), ws.numel(), stream))

            forms = {"max_concentrations": lambda: check(lib.sx_stain_max_concentrations(x.data_ptr(), code, n, size, size, None, 0, he.data_ptr(), 1, max_c.data_ptr(), pixels.data_ptr(), 0,
                                                                                          ws.data_ptr(), ws.numel(), stream)),
                     "luminosity_percentile": percentile(lib.sx_luminosity_percentile, 0),
                     "luminosity_percentile_pooled": percentile(lib.sx_luminosity_percentile, 1),
                     "luminosity_percentile_no_runs": percentile(diag.sx_luminosity_percentile_plain, 0),
                     "luminosity_percentile_with_runs_diag_build": percentile(diag.sx_luminosity_percentile, 0),
                     "reinhard_apply_stats": lambda: check(lib.sx_reinhard_apply_stats(x.data_ptr(), out.data_ptr(), code, n, size, size, src_mean.data_ptr(), src_std.data_ptr(), n,
                                                                                       ref_mean.data_ptr(), ref_std.data_ptr(), stream)),
                     "luminosity_apply": lambda: check(lib.sx_luminosity_apply(x.data_ptr(), out.data_ptr(), code, n, size, size, lum.data_ptr(), n, stream)),
                     "reinhard_tile_transform": lambda: reinhard.transform(x),
                     "luminosity_forward": lambda: std(x)}
            for fn in forms.values():      # warm-up (the percentile is in `lum` before the apply pass is timed)
                for _ in range(3):
                    fn()
            forms["luminosity_percentile"]()
            torch.cuda.synchronize()
            times = {form: [] for form in forms}
            for _ in range(args.repeats):      # alternated: one window of each form per repeat
                for form, fn in forms.items():
                    if form == "luminosity_apply":
                        forms["luminosity_percentile"]()      # (the pooled form left one row)
                    times[form].append(window(fn, args.calls))
            row = {"dtype": str(dtype).replace("torch.", ""), "batch": kind, "shape": [n, 3, size, size], "calls_per_window": args.calls, "percentile": 95.0,
                   "share_of_most_common_pixel": float((tiles == torch.tensor(GLASS, dtype=torch.uint8).view(1, 3, 1, 1)).all(dim=1).float().mean()),
                   "lightness_percentile_min_max": [float(std.estimate(x).lightness.min()), float(std.estimate(x).lightness.max())]}
            for form, values in times.items():
                row[form] = {"mean_us": float(np.mean(values)), "min_us": float(np.min(values)), "max_us": float(np.max(values))}
            mean = {form: row[form]["mean_us"] for form in forms}
            row["percentile_to_max_concentrations"] = mean["luminosity_percentile"] / mean["max_concentrations"]
            row["no_runs_to_with_runs_same_build"] = mean["luminosity_percentile_no_runs"] / mean["luminosity_percentile_with_runs_diag_build"]
            row["apply_to_reinhard_apply_stats"] = mean["luminosity_apply"] / mean["reinhard_apply_stats"]
            row["forward_to_reinhard_tile_transform"] = mean["luminosity_forward"] / mean["reinhard_tile_transform"]
            results.append(row)
            print(json.dumps(row))
    by = {(r["dtype"], r["batch"]): r for r in results}
    ratios = {dt: {"percentile_glass_to_tissue": by[(dt, "glass")]["luminosity_percentile"]["mean_us"] / by[(dt, "tissue")]["luminosity_percentile"]["mean_us"],
                   "percentile_no_runs_glass_to_tissue": by[(dt, "glass")]["luminosity_percentile_no_runs"]["mean_us"] / by[(dt, "tissue")]["luminosity_percentile_no_runs"]["mean_us"]}
              for dt in ("uint8", "float32")}
    print(json.dumps(ratios))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(dev), "results": results, "glass_to_tissue": ratios}, indent=1) + "\n")


if __name__ == "__main__":
    main()
