"""Host time of the Python layers per call: the microseconds a call of the binding (stainx_amd/backends/torch_hip_backend.py) or of a public
front end above it spends before it returns, for comparing two versions of either layer on the same shared objects.
    PYTHONPATH=<checkout> python tools/binding_host_time.py --out FILE.json [--blocks 40] [--calls 250]
    python tools/binding_host_time.py --table PARENT1.json AFTER1.json PARENT2.json AFTER2.json [PARENT3.json AFTER3.json ...]
Every case makes blocks of back-to-back calls at 2 x 3 x 48 x 48 (the device keeps up at that size: the clock sees the enqueue), one
synchronize behind each block, and reports the median over the blocks of the block's time per call.  Run the versions as child
processes in turn, parent, after, parent, after, ...: the parent runs give the spread of the measurement on that host on that day (whole
processes differ by several per cent), and --table holds every case's `after` median to the largest parent median plus that spread."""
import argparse, json, statistics, sys, time

import torch


def cases(dev):
    import stainx_amd as sx
    from stainx_amd import distributed as sxd, synth
    from stainx_amd.backends import torch_hip_backend as B

    u8 = synth.he_batch(2, 48, 48, seed0=1000).to(dev)
    f32 = synth.as_dtype(u8.cpu(), torch.float32).to(dev)
    mac, dec, rei, hm = B.MacenkoHIP(dev), B.DeconvHIP(dev), B.ReinhardHIP(dev), B.HistogramMatchingHIP(dev)
    he, max_c = mac.compute_reference_stain_matrix(synth.reference_tile(48, 48).to(dev))
    est = mac.estimate(u8)
    src_he, src_mc = est["he"].contiguous(), est["max_c"].contiguous()
    hed = torch.tensor([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]).t().contiguous().to(dev)
    mean, std = torch.tensor([150.0, 140.0, 120.0], device=dev), torch.tensor([20.0, 8.0, 9.0], device=dev)
    rows_mean, rows_std = mean.expand(2, 3).contiguous(), std.expand(2, 3).contiguous()
    hist = hm.compute_reference_histograms(u8)
    tables = (torch.arange(256, dtype=torch.float32, device=dev) / 255).repeat(1, 3, 1).contiguous()
    def gen():
        return torch.Generator(device=dev).manual_seed(1)      # (on the device: a draw enqueues no host copy)

    distribution = sx.StatisticsDistribution(mean, std / 4, std, std / 4)
    deconv, hed_aug, hsv_aug, mac_aug = sx.ColorDeconvolution("hed"), sx.HEDAugment(generator=gen()), sx.HSVAugment(generator=gen()), sx.MacenkoAugment(generator=gen())
    stat_aug, lum = sx.StatisticsAugment(distribution, "lab", generator=gen()), sx.LuminosityStandardizer()
    reinhard, matching = sx.Reinhard(device=dev).fit(u8), sx.HistogramMatching(device=dev).fit(u8)
    return {
        "MacenkoHIP.transform uint8": lambda: mac.transform(u8, he, max_c),
        "MacenkoHIP.transform float32": lambda: mac.transform(f32, he, max_c),
        "MacenkoHIP.apply": lambda: mac.apply(u8, src_he, src_mc, he, max_c),
        "MacenkoHIP.separate_apply": lambda: mac.separate_apply(u8, src_he, src_mc, he, max_c),
        "DeconvHIP.apply": lambda: dec.apply(u8, hed),
        "ReinhardHIP.transform": lambda: rei.transform(u8, mean, std),
        "ReinhardHIP.apply_statistics": lambda: rei.apply_statistics(u8, rows_mean, rows_std, mean, std),
        "HistogramMatchingHIP.transform": lambda: hm.transform(u8, hist),
        "HistogramMatchingHIP.apply_tables": lambda: hm.apply_tables(u8, tables),
        "tissue_mask_native": lambda: B.tissue_mask_native(u8, 0.8, False),
        "pooled fit_transform step (distributed, one rank)": lambda: sxd.macenko_fit_transform_pooled(f32, steps=mac),
        # the front ends: their own checks in front of the binding's call(s)
        "ColorDeconvolution.apply": lambda: deconv.apply(u8),
        "HEDAugment": lambda: hed_aug(u8),
        "HSVAugment": lambda: hsv_aug(u8),
        "MacenkoAugment": lambda: mac_aug(u8),
        "StatisticsAugment (lab)": lambda: stat_aug(u8),
        "LuminosityStandardizer": lambda: lum(u8),
        "Reinhard.apply": lambda: reinhard.apply(u8, (rows_mean, rows_std)),
        "HistogramMatching.apply": lambda: matching.apply(u8, tables),
        "tissue_mask": lambda: sx.tissue_mask(u8),
        "focus_statistics": lambda: sx.focus_statistics(u8),
        "sample_pixels": lambda: sx.sample_pixels(u8, 64),
    }


def measure(out, blocks, calls):
    dev = torch.device("cuda", 0)
    result = {}
    for name, call in cases(dev).items():
        for _ in range(calls):      # warm: allocator, scratch, ctypes' function objects
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(blocks):
            t0 = time.perf_counter_ns()
            for _ in range(calls):
                call()
            t1 = time.perf_counter_ns()
            torch.cuda.synchronize()
            per_call.append((t1 - t0) / calls)
        result[name] = {"median_ns": statistics.median(per_call), "min_ns": min(per_call)}
        print(f"{name}: {result[name]['median_ns'] / 1000:.2f} us", flush=True)
    with open(out, "w") as f:
        json.dump(result, f, sort_keys=True, indent=1)
        f.write("\n")


def table(paths):
    runs = [json.load(open(p)) for p in paths]      # parent, after, parent, after, ...
    parents, afters = runs[0::2], runs[1::2]
    print(f"host time per call, median over blocks, microseconds; {len(parents)} rounds of parent, after in turn")
    print("bound: the largest parent median plus the spread of the parent medians; after: the median of the after runs")
    for name in runs[0]:
        p = [r[name]["median_ns"] / 1000 for r in parents]
        a = [r[name]["median_ns"] / 1000 for r in afters]
        bound, after = max(p) + (max(p) - min(p)), statistics.median(a)
        print(f"{name}\n    parent {' '.join(f'{v:7.2f}' for v in p)}   (median {statistics.median(p):.2f})\n    after  {' '.join(f'{v:7.2f}' for v in a)}   (median {after:.2f})"
              f"\n    bound {bound:.2f}: {'within' if after <= bound else 'ABOVE'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--calls", type=int, default=250)
    ap.add_argument("--table", nargs="+", metavar="JSON")
    args = ap.parse_args()
    if args.table:
        table(args.table)
    elif args.out:
        measure(args.out, args.blocks, args.calls)
    else:
        sys.exit("give --out FILE.json or --table with the files of the runs")
