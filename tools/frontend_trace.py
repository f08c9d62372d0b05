"""What the public front ends ask of the library, call by call, for comparing two versions of the Python layer above the binding (deconv.py,
hsv.py, augment.py, statistics_augment.py, luminosity.py, masks.py, focus.py, sampling.py, normalizers/*.py) on the SAME shared objects:
    PYTHONPATH=<checkout> STAINX_HIP_LIB=<libstainx_hip.so> python tools/frontend_trace.py --out FILE.json
tools/binding_trace.py's recording pass-through and its description of a result, one layer up: a fixed list of calls at 2 x 3 x 48 x 48 -- every
public call of those files, each on fresh objects, in uint8, bfloat16 and float32, planar and (where taken) NHWC, unmasked, with the
luminosity rule and with an explicit mask, on a single CHW tile with its (H, W) mask, with N = 0, and the four augmentation modules drawing
from a seeded generator on the CPU and on the device.  One line per call: how often it ran, the library's entry points reached, one sha256
over the traces and over shape / dtype / sha256 of everything returned (or the refusal).  Two versions of the same behaviour give
byte-identical files.  Evidence for a change, not a test: nothing is asserted."""
import argparse, json

import torch

import binding_trace as bt      # (tools/ is on the path of a script run from it; importing it fits its shared references on the device)
from binding_trace import Recorder, describe, mask_of

import stainx_amd as sx
from stainx_amd import _native, synth

DEV, U8, BF16, F32 = bt.DEV, bt.U8, bt.BF16, bt.F32
ALL = (U8, BF16, F32)
REF = synth.reference_tile(48, 48).to(DEV)      # (1, 3, 48, 48) uint8
LAB, HED = (torch.tensor([150.0, 140.0, 120.0]), torch.tensor([20.0, 8.0, 9.0])), (torch.tensor([0.5, 0.3, 0.1]), torch.tensor([0.2, 0.1, 0.05]))
DIST = sx.StatisticsDistribution(LAB[0], LAB[1] / 4, LAB[1], LAB[1] / 4)
HED_DIST = sx.StatisticsDistribution(HED[0], HED[1] / 4, HED[1], HED[1] / 4)


def n_of(x):
    return 1 if x.dim() == 3 else x.shape[0]


def axis(last):
    return -1 if last else 1


def rows(x, k, seed, lo=0.8, hi=1.2):
    return bt.rows(n_of(x), k, seed, lo, hi)


def generators():
    return (None, torch.Generator().manual_seed(7), torch.Generator(device=DEV).manual_seed(7))


def planar(x, last):
    x = x if x.dim() == 4 else x.unsqueeze(0)
    return x.permute(0, 3, 1, 2) if last else x


def fitted(cls, **options):
    return cls(device=DEV, **options).fit(REF if options.get("channel_axis", 1) == 1 else REF.permute(0, 2, 3, 1).contiguous())


def parts(value):
    """A dataclass or named tuple as a plain list (``describe`` knows tensors, lists and dicts)."""
    return list(value) if isinstance(value, tuple) else [getattr(value, f) for f in value.__dataclass_fields__]


def hsv_rows(x):
    return torch.tensor([0.03, 1.1, -0.02, 0.9, 0.05]).repeat(n_of(x), 1).to(DEV)


def drawn(make):
    """An augmentation module per generator (none: explicit factors are the caller's; a CPU one; one on the device), seeded alike."""
    torch.manual_seed(11)
    return [make(g) for g in generators()[1:]]


def sampled():
    """The four modules' draws for 3 tiles on the device: the default generator (seeded here), a CPU generator, one on the device."""
    torch.manual_seed(13)
    own = (LAB[0].expand(3, 3), LAB[1].expand(3, 3))
    return [[sx.HEDAugment(generator=g).sample_factors(3, DEV), sx.MacenkoAugment(generator=g).sample_factors(3, DEV), sx.HSVAugment(p=0.5, generator=g).sample_rows(3, DEV),
             sx.StatisticsAugment(DIST, kind="laplace", p=0.5, generator=g).sample_targets(3, DEV, own=own)] for g in generators()]


# label -> (dtypes, takes NHWC, takes mask=, takes a CHW tile, call(x, last, m));  m: None, "luminosity" or an explicit mask
D, M, R, H, V = sx.ColorDeconvolution, sx.Macenko, sx.Reinhard, sx.HistogramMatching, sx.Vahadane
CASES = {
    "ColorDeconvolution.separate": (ALL, True, False, True, lambda x, last, m: parts(D("hed", channel_axis=axis(last)).separate(x, concentrations=True))[:2]),
    "ColorDeconvolution.apply": (ALL, True, True, True, lambda x, last, m: [D("hed", target=t, channel_axis=axis(last), normalize_to_0_1=z).apply(x, a, a, mask=m) for t in (None, "hdab") for z in (False, True) for a in (None, rows(x, 3, 5))]),
    "ColorDeconvolution(mask=).apply": (ALL, False, False, True, lambda x, last, m: D("hed", mask="luminosity", luminosity_threshold=0.7).apply(x)),
    "ColorDeconvolution.quantify": (ALL, True, True, True, lambda x, last, m: [parts(D("hdab", channel_axis=axis(last)).quantify(x, pooled=p, bin_log2=4, zero_bin=32, mask=m))[:3] for p in (False, True)]),
    "ColorDeconvolution.estimate": (ALL, True, True, True, lambda x, last, m: [parts(D("hed", channel_axis=axis(last)).estimate(x, pooled=p, mask=m)) for p in (False, True)]),
    "ColorDeconvolution.match": (ALL, True, True, True, lambda x, last, m: [D("hed", channel_axis=axis(last)).match(x, s, (HED[0].to(DEV), HED[1]), mask=m) for s in (HED, D("hed", channel_axis=axis(last)).estimate(x, mask=m))]),
    "ColorDeconvolution.combine": ((F32,), True, False, True, lambda x, last, m: [D("hed", channel_axis=axis(last)).combine(x, out_dtype=o) for o in (U8, BF16, F32)]),
    "HEDAugment": (ALL, False, True, True, lambda x, last, m: [sx.HEDAugment()(x, rows(x, 3, 1), rows(x, 3, 2, -0.1, 0.1), mask=m)] + [a(x, mask=m) for a in drawn(lambda g: sx.HEDAugment(0.1, (0.1, 0.2, 0.0), basis="hdab", generator=g))]),
    "adjust_hsv": (ALL, True, True, True, lambda x, last, m: [sx.adjust_hsv(x, r, mask=m, channel_axis=axis(last), normalize_to_0_1=z) for r in (hsv_rows(x), hsv_rows(x[:1])[0]) for z in (False, True)]),
    "adjust_hsv out_dtype": ((U8,), True, False, True, lambda x, last, m: [sx.adjust_hsv(x, hsv_rows(x), channel_axis=axis(last), out_dtype=o) for o in (BF16, torch.float16)]),
    "HSVAugment": (ALL, False, True, True, lambda x, last, m: [sx.HSVAugment()(x, hsv_rows(x), mask=m)] + [a(x, mask=m) for a in drawn(lambda g: sx.HSVAugment(0.1, 0.2, 0.2, value_shift=0.05, p=0.5, generator=g))]),
    "HSVAugment(mask=)": ((U8,), False, False, True, lambda x, last, m: sx.HSVAugment(mask="luminosity", generator=torch.Generator().manual_seed(3))(x)),
    "MacenkoAugment": (ALL, False, True, True, lambda x, last, m: [sx.MacenkoAugment()(x, rows(x, 2, 1), rows(x, 2, 2, -0.1, 0.1), mask=m)] + [a(x, mask=m) for a in drawn(lambda g: sx.MacenkoAugment(generator=g))]),
    "MacenkoAugment(reference=)": ((U8, F32), False, True, True, lambda x, last, m: [a(x, mask=m) for a in drawn(lambda g: sx.MacenkoAugment(reference=REF, generator=g, normalize_to_0_1=False))]),
    "MacenkoAugment(source=)": ((U8, F32), False, True, True, lambda x, last, m: [sx.MacenkoAugment(source=M(device=DEV).estimate(planar(x, last), pooled=True), normalizer=n, generator=torch.Generator().manual_seed(5))(x, mask=m) for n in (None, fitted(M))]),
    "StatisticsAugment lab": (ALL, False, True, True, lambda x, last, m: [sx.StatisticsAugment(DIST)(x, (LAB[0], LAB[1].to(DEV)), mask=m)] + [a(x, mask=m) for k in sx.statistics_augment.KINDS for a in drawn(lambda g: sx.StatisticsAugment(DIST, kind=k, p=0.5, generator=g))]),
    "StatisticsAugment hed": (ALL, False, True, True, lambda x, last, m: [sx.StatisticsAugment(HED_DIST, "hed")(x, HED, mask=m)] + [a(x, mask=m) for k in sx.statistics_augment.KINDS for a in drawn(lambda g: sx.StatisticsAugment(HED_DIST, "hed", kind=k, p=0.5, basis="he", generator=g))]),
    "StatisticsAugment(mask=)": ((U8,), False, False, True, lambda x, last, m: [sx.StatisticsAugment(d, s, mask="luminosity", generator=torch.Generator().manual_seed(3))(x) for d, s in ((DIST, "lab"), (HED_DIST, "hed"))]),
    "sample_factors / sample_rows / sample_targets": ((U8,), False, False, False, lambda x, last, m: sampled()),
    "LuminosityStandardizer": (ALL, False, False, True, lambda x, last, m: [sx.LuminosityStandardizer(90.0, s)(x) for s in ("tile", "batch")]),
    "LuminosityStandardizer explicit mask": (ALL, False, False, True, lambda x, last, m: [sx.LuminosityStandardizer()(x, mask=mask_of(planar(x, last), False).reshape(x.shape[:-3] + x.shape[-2:])),
                                                                                             parts(sx.LuminosityStandardizer().estimate(x, pooled=True, mask=mask_of(planar(x, last), False).bool().reshape(x.shape[:-3] + x.shape[-2:])))]),
    "LuminosityStandardizer.estimate + apply": (ALL, False, False, True, lambda x, last, m: [sx.LuminosityStandardizer().apply(x, e) for e in (sx.LuminosityStandardizer().estimate(x), sx.LuminosityStandardizer().estimate(x, pooled=True).luminance)]),
    "tissue_mask": (ALL, True, False, False, lambda x, last, m: sx.tissue_mask(x, 0.7, channel_axis=axis(last))),
    "luminosity_histogram": (ALL, True, False, False, lambda x, last, m: [parts(sx.luminosity_histogram(x, pooled=p, channel_axis=axis(last))) for p in (False, True)]),
    "otsu_mask": (ALL, True, False, False, lambda x, last, m: [parts(sx.otsu_mask(x, pooled=p, channel_axis=axis(last), open_radius=1, close_radius=2, min_object_area=4, min_hole_area=4)) for p in (False, True)]),
    "mask_morphology / refine_mask": ((U8,), False, False, False, lambda x, last, m: [sx.mask_morphology(mask_of(x, False), op, 2, element=e) for op in sx.masks.MORPHOLOGY_OPS for e in sx.masks.MORPHOLOGY_ELEMENTS]
                                      + [sx.refine_mask(mask_of(x, False).unsqueeze(1)), sx.refine_mask(mask_of(x, False).bool(), open_radius=1, element="square", min_hole_area=9, connectivity=4)]),
    "mask_components / area filters": ((U8,), False, False, False, lambda x, last, m: [parts(sx.mask_components(mask_of(x, False), connectivity=c, holes=h)) for c in (4, 8) for h in (False, True)]
                                       + [sx.remove_small_objects(mask_of(x, False), 5), sx.remove_small_holes(mask_of(x, False).bool(), 5, connectivity=4)]),
    "saturation_map + median_filter + level_*": (ALL, True, False, False, lambda x, last, m: (lambda s: [s, sx.median_filter(s, 5), parts(sx.level_histogram(s, pooled=True)), sx.otsu_level(sx.level_histogram(s)), sx.level_mask(s, 20),
                                                                                                       sx.level_mask(s.unsqueeze(1), torch.full((n_of(x),), 30))])(sx.saturation_map(x, channel_axis=axis(last)))),
    "saturation_mask": (ALL, True, False, False, lambda x, last, m: [parts(sx.saturation_mask(x, threshold=t, median_size=s, pooled=p, channel_axis=axis(last), close_radius=1)) for t, s, p in ((None, 7, False), (None, 0, True), (8, 3, False))]),
    "grey_map": (ALL, True, False, False, lambda x, last, m: sx.grey_map(x, channel_axis=axis(last))),
    "focus_statistics": (ALL, True, True, False, lambda x, last, m: [parts(sx.focus_statistics(x, block=b, mask=m, pooled=p, channel_axis=axis(last))) for b, p in ((None, False), (None, True), ((16, 16), False), ((64, 8), False))]),
    "focus_mask + cells_mask": (ALL, True, True, False, lambda x, last, m: [parts(d)[:2] + parts(d.statistics) for d in (sx.focus_mask(x, 50.0, block=(16, 16), mask=m, channel_axis=axis(last)), sx.focus_mask(x, 5.0, block=(8, 32), min_pixels=1, mask=m, channel_axis=axis(last)))]),
    "sample_pixels": (ALL, True, True, False, lambda x, last, m: [parts(sx.sample_pixels(x, s, mask=m, pooled=p, offset=o, channel_axis=axis(last))) for s, p, o in ((64, False, 0), ((8, 8), True, 5), (1 << 13, False, 0))]),
    "Reinhard.fit + transform": (ALL, False, True, False, lambda x, last, m: [R(device=DEV, statistics=s).fit(synth.as_dtype(REF.cpu(), x.dtype).to(DEV), mask=None if m is None else "luminosity").transform(x, mask=m) for s in ("batch", "tile")]),
    "Reinhard(mask=).fit_transform": (ALL, False, False, False, lambda x, last, m: R(device=DEV, mask="luminosity", luminosity_threshold=0.7).fit_transform(x)),
    "Reinhard.estimate + apply": (ALL, False, True, False, lambda x, last, m: [fitted(R).apply(x, R(device=DEV).estimate(x, pooled=p, mask=m), mask=m) for p in (False, True)] + [R(device=DEV).apply(x, LAB, mask=m, target=(LAB[0] + 5, LAB[1]))]),
    "HistogramMatching.fit + transform": (ALL, True, True, False, lambda x, last, m: [H(device=DEV, channel_axis=axis(last), statistics=s).fit(x, mask=m).transform(x, mask=m) for s in ("batch", "tile")]),
    "HistogramMatching.estimate + lookup_tables + apply": (ALL, True, True, False, lambda x, last, m: (lambda h: [parts(h.estimate(x, mask=m)), h.lookup_tables(h.estimate(x, pooled=True, mask=m)), h.apply(x, h.estimate(x, mask=m), mask=m),
                                                                                                          h.apply(x, h.lookup_tables(sx.HistogramStatistics.pool(h.estimate(x, mask=m))), mask=m)])(fitted(H, channel_axis=axis(last)))),
    "Macenko.fit + transform": (ALL, False, True, False, lambda x, last, m: [M(device=DEV, normalize_to_0_1=z).fit(REF, mask=None if m is None else "luminosity").transform(x, mask=m) for z in (False, True)]),
    "Macenko.separate": (ALL, False, True, False, lambda x, last, m: [parts(n.separate(x, concentrations=True, mask=m, source=s)) for n in (M(device=DEV), fitted(M)) for s in (None, M(device=DEV).estimate(x, mask=m))]),
    "Macenko.estimate + apply": (ALL, False, True, False, lambda x, last, m: [fitted(M, output_dtype=BF16 if x.dtype == U8 else None).apply(x, M(device=DEV).estimate(x, pooled=p, mask=m), mask=m) for p in (False, True)]
                                 + [M(device=DEV).apply(x, M(device=DEV).estimate(x), alpha=rows(x, 2, 3), beta=rows(x, 2, 4, -0.1, 0.1), own_basis=True, mask=m)]),
    "Vahadane.fit + transform": (ALL, False, True, False, lambda x, last, m: V(device=DEV, iterations=4).fit(REF, mask=m if isinstance(m, str) else None).transform(x, mask=m)),
    "Vahadane(mask=None)": ((U8, F32), False, False, False, lambda x, last, m: [parts(V(device=DEV, iterations=4, mask=None).estimate(x, pooled=p)) for p in (False, True)]),
    "Vahadane.estimate + max_concentrations + separate": (ALL, False, True, False, lambda x, last, m: (lambda v: [parts(v.estimate(x, pooled=True, mask=m))[:2], v.max_concentrations(x, v.estimate(x, mask=m), mask=m),
                                                                                                         parts(v.separate(x, concentrations=True, mask=m))])(V(device=DEV, iterations=4, init=bt.FIT[0]))),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true", help="every trace and every description in full (large)")
    args = ap.parse_args()
    _native._lib = Recorder(_native.require())
    entries = []
    for label, (dtypes, nhwc, masks, tile, call) in CASES.items():
        runs = [(dt, last, mode, "full") for dt in dtypes for last in ((False, True) if nhwc else (False,)) for mode in (("none", "rule", "explicit") if masks and not last else ("none",))]
        runs += [(dtypes[0], False, "explicit" if masks else "none", "N=0")] + ([(dt, last, "explicit" if masks and not last else "none", "tile") for dt in dtypes[::2] for last in ((False, True) if nhwc else (False,))] if tile else [])
        for dt, last, mode, variant in runs:
            x = bt.batch(dt, last, "N=0" if variant == "N=0" else "full")
            m = {"none": None, "rule": "luminosity", "explicit": mask_of(x, last)}[mode]
            if variant == "tile":
                x, m = x[0], m[0] if isinstance(m, torch.Tensor) else m
            entries.append(bt.record(f"{label} | {str(dt)[6:]} {'NHWC' if last else 'NCHW'} mask: {mode} {variant}", lambda: call(x, last, m)))
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in (entries if args.full else bt.digest(entries))) + "\n]\n")
    for e in entries:
        if "raises" in e:
            print(f"raised: {e['call']}: {e['raises'][:200]}")
    print(f"{len(entries)} calls recorded, {sum('raises' in e for e in entries)} of them raised -> {args.out}")


if __name__ == "__main__":
    main()
