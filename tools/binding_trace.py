"""What the Python binding asks of the library, call by call, for comparing two versions of stainx_amd/backends/torch_hip_backend.py on
the SAME shared objects (a refactor of the binding against its parent):
    PYTHONPATH=<checkout> STAINX_HIP_LIB=<libstainx_hip.so> python tools/binding_trace.py --out FILE.json
Both libraries are replaced by a recording pass-through: for every entry point called it writes down the name, each scalar argument
exactly, each pointer argument as null / ptr (a workspace's byte count is a scalar) and the value returned.  A fixed list of calls at
2 x 3 x 48 x 48 -- every public method of the backend classes and the eleven *_native functions, each on a fresh object, in the dtypes
and layouts it takes, with an explicit mask and the rule's, with N = 0 and H = 0, and the single-fault refused calls -- is recorded as
trace + shape / dtype / sha256 of every tensor returned, or the exception.  The file holds one line per method -- its calls counted,
the entry points they reached, one sha256 over their traces and results -- and every refusal in full (--full: every call in full).
Two versions of the same behaviour give byte-identical files.  Evidence for a change, not a test: nothing is asserted."""
import argparse, hashlib, json
from ctypes import c_void_p

import torch
from stainx_amd import _native, distributed as sxd, synth
from stainx_amd.backends import torch_hip_backend as B

DEV = torch.device("cuda", 0)
U8, BF16, F32 = torch.uint8, torch.bfloat16, torch.float32
LOG: list = []


class Recorder:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = _native.SIGNATURES.get(name) or _native.DIAG_SIGNATURES.get(name)
        if sig is None or name == "sx_last_error_string":
            return fn

        def call(*args):
            res = fn(*args)
            shown = [("null" if a is None or a == 0 else "ptr") if t is c_void_p else a for a, t in zip(args, sig[1])]
            LOG.append([name, shown, res if isinstance(res, (int, float)) else None])
            return res
        return call


def describe(value):
    if isinstance(value, torch.Tensor):
        flat = torch.empty(value.numel(), dtype=value.dtype)      # (a fresh dense copy: a one-element view keeps its parent's stride)
        data = flat.copy_(value.detach().reshape(-1)).view(U8).numpy().tobytes()
        return {"shape": list(value.shape), "dtype": str(value.dtype), "sha256": hashlib.sha256(data).hexdigest()}
    if isinstance(value, dict):
        return {k: describe(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [describe(v) for v in value]
    return value


def batch(dtype, last=False, variant="full"):
    x = synth.as_dtype(synth.he_batch(2, 48, 48, seed0=1000), dtype)
    x = {"full": x, "N=0": x[:0], "H=0": x[:, :, :0]}[variant]
    return (x.permute(0, 2, 3, 1) if last else x).contiguous().to(DEV)


def mask_of(x, last):
    planar = x.permute(0, 3, 1, 2) if last else x
    return (planar.float().mean(dim=1) < (200.0 if x.dtype == U8 else 200.0 / 255)).to(U8).contiguous()


def rows(n, k, seed, lo=0.8, hi=1.2):
    return (lo + (hi - lo) * torch.rand(n, k, generator=torch.Generator().manual_seed(seed))).to(DEV)


# the fitted references every call shares (made before the recorders are in place)
FIT = B.MacenkoHIP(DEV).compute_reference_stain_matrix(synth.reference_tile(48, 48).to(DEV))
HED = torch.tensor([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]).t().contiguous()
LAB = (torch.tensor([150.0, 140.0, 120.0]), torch.tensor([20.0, 8.0, 9.0]))
HIST = [h.contiguous() for h in torch.softmax(torch.rand(3, 256, generator=torch.Generator().manual_seed(11)), dim=1).to(DEV)]
TABLES = (torch.arange(256, dtype=F32) / 255).flip(0).repeat(1, 3, 1)
M, V, L, D, R, H = B.MacenkoHIP, B.VahadaneHIP, B.LuminosityHIP, B.DeconvHIP, B.ReinhardHIP, B.HistogramMatchingHIP


def source(x, n):
    est = M(DEV).estimate(x)
    return est["he"][:n], est["max_c"][:n]


def dfit(x):
    be = M(DEV)
    state = be.dfit_begin(be.dfit_moments(x))
    for stage in (0, 1):
        for _ in range(4):
            be.dfit_advance(state, stage, be.dfit_histogram(x, state, stage))
    return be.dfit_result(state)


def pfit_packed(x):
    be = M(DEV)
    n, _, h, w = x.shape
    counts = [be.pfit_sample_count(n, h, w)]
    got, n_all, sample = be.pfit_stats_packed(x).unsqueeze(0), n * h * w, min(4096, counts[0])
    stale = be.pfit_plane_packed(got, counts, None, n_all, sample, (n, h, w))
    for stage in (0, 1):
        row = be.pfit_gather_packed(be.pfit_pass(x, stage, n_all, sample), stage, n_all, sample, (n, h, w), 32768, stale)
        out = be.pfit_finish_packed(row.unsqueeze(0), stage, n_all, sample, (n, h, w), 32768)
    return out, be.pfit_empty_record(), params(1)(be)


def same_storage(x):
    he, mc = (t.clone() for t in source(x, 1))
    out = M(DEV).separate_apply(x, he, mc, *FIT)
    return out["he"].untyped_storage().data_ptr() == he.untyped_storage().data_ptr() and out["max_c"].untyped_storage().data_ptr() == mc.untyped_storage().data_ptr()


def then(be, call, *readers):
    """The call's result, then what the object's readers (a method's name, or a function of the object) say afterwards."""
    return [call(be)] + [getattr(be, r)() if isinstance(r, str) else r(be) for r in readers]


def params(n):      # (the stage stamps of the diagnostic build are times: left out)
    return lambda be: [be.last_workspace.numel(), {k: v for k, v in be.tile_params(n).items() if k in ("n_kept", "he", "max_c")}]


# label -> (dtypes, has NHWC, has mask / None, call(x, last, mask));  x: the batch, last: its layout, mask: explicit or None
ALL, N, n_of = (U8, BF16, F32), None, lambda x: x.shape[0]
CASES = {
    "Macenko.transform": (ALL, True, False, lambda x, last, m: then(M(DEV), lambda be: be.transform(x, *FIT, channels_last=last), params(n_of(x)))),
    "Macenko.transform out_dtype": ((U8,), True, False, lambda x, last, m: [M(DEV).transform(x, *FIT, channels_last=last, out_dtype=o, normalize_to_0_1=z) for o in (BF16, torch.float16, N) for z in (False, True)]),
    "Macenko.transform sampled": ((U8, F32), False, False, lambda x, last, m: M(DEV, precision="sampled").transform(x, *FIT)),
    "Macenko.augment": (ALL, True, False, lambda x, last, m: [M(DEV).augment(x, rows(n_of(x), 2, 1), rows(n_of(x), 2, 2, -0.1, 0.1), *ref, channels_last=last) for ref in ((), FIT)]),
    "Macenko.separate": (ALL, True, False, lambda x, last, m: [M(DEV).separate(x, *ref, concentrations=True, max_conc=True, channels_last=last) for ref in ((), FIT)]),
    "Macenko.estimate": (ALL, True, False, lambda x, last, m: M(DEV).estimate(x, channels_last=last)),
    "Macenko.apply": (ALL, True, False, lambda x, last, m: [M(DEV).apply(x, *source(x.permute(0, 3, 1, 2) if last else x, k), *FIT, alpha=a, beta=a, channels_last=last) for k in (1, 2) for a in (N, rows(n_of(x), 2, 3))]),
    "Macenko.apply own basis": ((U8,), False, False, lambda x, last, m: M(DEV).apply(x, source(x, 2)[0], N, alpha=rows(n_of(x), 2, 3), beta=rows(n_of(x), 2, 4, -0.1, 0.1), out_dtype=BF16)),
    "Macenko.estimate_masked": (ALL, False, True, lambda x, last, m: [M(DEV).estimate_masked(x, m, pooled=p) for p in (False, True)]),
    "Macenko.compute_reference_stain_matrix_masked": ((U8, F32), False, True, lambda x, last, m: M(DEV).compute_reference_stain_matrix_masked(x, m)),
    "Macenko.transform_masked": (ALL, False, True, lambda x, last, m: M(DEV).transform_masked(x, *FIT, m, normalize_to_0_1=True)),
    "Macenko.apply_masked": (ALL, False, True, lambda x, last, m: M(DEV).apply_masked(x, *source(x, 2), *FIT, m, alpha=rows(n_of(x), 2, 3), beta=rows(n_of(x), 2, 4, -0.1, 0.1))),
    "Macenko.separate_apply": (ALL, True, False, lambda x, last, m: [M(DEV).separate_apply(x, *source(x.permute(0, 3, 1, 2) if last else x, k), *ref, concentrations=True, channels_last=last) for k in (1, 2) for ref in ((), FIT)]),
    "Macenko.separate_apply same tensors": ((U8,), False, False, lambda x, last, m: bool(same_storage(x))),
    "Macenko.separate_apply_masked": (ALL, False, True, lambda x, last, m: M(DEV).separate_apply_masked(x, *source(x, 2), *FIT, m, concentrations=True)),
    "Macenko.separate_masked": (ALL, False, True, lambda x, last, m: [M(DEV).separate_masked(x, *ref, m, concentrations=True, max_conc=True) for ref in ((N, N), FIT)]),
    "Macenko.augment_masked": (ALL, False, True, lambda x, last, m: [M(DEV).augment_masked(x, rows(n_of(x), 2, 1), rows(n_of(x), 2, 2, -0.1, 0.1), *ref, m) for ref in ((N, N), FIT)]),
    "Macenko.compute_reference_stain_matrix + tile_params": ((U8, F32), False, False, lambda x, last, m: then(M(DEV), lambda be: be.compute_reference_stain_matrix(x), params(1))),
    "Macenko.dfit_*": ((U8, F32), False, False, lambda x, last, m: dfit(x)),
    "Macenko.pfit_* (distributed, one rank)": ((U8, F32), False, False, lambda x, last, m: sxd.macenko_fit_pooled(x, steps=M(DEV))),
    "Macenko.pfit_*_packed": ((U8, F32), False, False, lambda x, last, m: pfit_packed(x)),
    "Vahadane.vahadane_estimate": (ALL, False, True, lambda x, last, m: [V(DEV).vahadane_estimate(x, FIT[0].reshape(1, 3, 2), iterations=4, pooled=p, masked=k, mask=m) for p in (False, True) for k in (False, True)]),
    "Vahadane.max_concentrations": (ALL, False, True, lambda x, last, m: [V(DEV).max_concentrations(x, FIT[0], pooled=p, masked=k, mask=m) for p in (False, True) for k in (False, True)]),
    "Luminosity.percentile": (ALL, False, True, lambda x, last, m: [L(DEV).percentile(x, 95.0, pooled=p, mask=m) for p in (False, True)]),
    "Luminosity.apply": (ALL, False, False, lambda x, last, m: [L(DEV).apply(x, torch.full((k,), 0.9)) for k in (1, n_of(x))]),
    "Deconv.apply": (ALL, True, False, lambda x, last, m: [D(DEV).apply(x, HED, t, alpha=a, beta=a, channels_last=last) for t in (N, HED.unsqueeze(0)) for a in (N, rows(n_of(x), 3, 5))]),
    "Deconv.apply masked": (ALL, False, True, lambda x, last, m: D(DEV).apply(x, HED, masking=(m, 0.8), normalize_to_0_1=True)),
    "Deconv.separate": (ALL, True, False, lambda x, last, m: [D(DEV).separate(x, HED, stains=s, concentrations=True, channels_last=last) for s in (False, True)]),
    "Deconv.combine": ((F32,), True, False, lambda x, last, m: [D(DEV).combine(x, HED, out_dtype=o, channels_last=last) for o in (U8, BF16, F32)]),
    "Deconv.quantify": (ALL, True, False, lambda x, last, m: [D(DEV).quantify(x, HED, per_tile=p, channels_last=last) for p in (False, True)]),
    "Deconv.quantify masked": (ALL, False, True, lambda x, last, m: D(DEV).quantify(x, HED, bin_log2=4, zero_bin=8, masking=(m, 0.8))),
    "Deconv.moments": (ALL, True, False, lambda x, last, m: [D(DEV).moments(x, HED, per_tile=p, channels_last=last) for p in (False, True)]),
    "Deconv.moments masked": (ALL, False, True, lambda x, last, m: D(DEV).moments(x, HED, masking=(m, 0.8))),
    "Reinhard.compute_reference_mean_std": (ALL, False, False, lambda x, last, m: R(DEV).compute_reference_mean_std(x)),
    "Reinhard.transform + workspace_status": (ALL, False, False, lambda x, last, m: then(R(DEV), lambda be: [be.transform(x, *LAB), be.transform(x, *LAB)], "workspace_status")),
    "Reinhard.tile_statistics": (ALL, False, False, lambda x, last, m: R(DEV).tile_statistics(x)),
    "Reinhard.transform_tiles": (ALL, False, False, lambda x, last, m: [R(DEV).transform_tiles(x, *LAB, return_statistics=s) for s in (False, True)]),
    "Reinhard.apply_statistics": (ALL, False, False, lambda x, last, m: [R(DEV).apply_statistics(x, LAB[0].expand(k, 3), LAB[1].expand(k, 3), *LAB) for k in (1, n_of(x))]),
    "Reinhard.masked_statistics": (ALL, False, True, lambda x, last, m: [R(DEV).masked_statistics(x, m, 0.8, per_tile=p) for p in (False, True)]),
    "Reinhard.transform_masked": (ALL, False, True, lambda x, last, m: [R(DEV).transform_masked(x, *LAB, m, 0.8, per_tile=p, return_statistics=p) for p in (False, True)]),
    "Reinhard.apply_statistics_masked": (ALL, False, True, lambda x, last, m: R(DEV).apply_statistics_masked(x, *LAB, *LAB, m, 0.8)),
    "Reinhard.apply_targets": (ALL, False, False, lambda x, last, m: R(DEV).apply_targets(x, *LAB, LAB[0].expand(n_of(x), 3), LAB[1].expand(n_of(x), 3))),
    "Reinhard.apply_targets_masked": (ALL, False, True, lambda x, last, m: R(DEV).apply_targets_masked(x, *LAB, *LAB, m, 0.8)),
    "Reinhard.local_sums + apply_with_sums": (ALL, False, False, lambda x, last, m: then(R(DEV), lambda be: be.apply_with_sums(x, be.local_sums(x), 2 * 48 * 48, *LAB))),
    "HM.compute_reference_histograms": (ALL, True, False, lambda x, last, m: H(DEV, channel_axis=-1 if last else 1).compute_reference_histograms(x)),
    "HM.transform + tables + workspace_status": (ALL, True, False, lambda x, last, m: then(H(DEV, channel_axis=-1 if last else 1), lambda be: [be.transform(x, HIST), be.transform(x, HIST[0])], "tables", "workspace_status")),
    "HM.transform_tiles + tile_tables": (ALL, True, False, lambda x, last, m: then(H(DEV, channel_axis=-1 if last else 1), lambda be: be.transform_tiles(x, HIST), "tile_tables")),
    "HM.compute_reference_histograms_masked": (ALL, False, True, lambda x, last, m: H(DEV).compute_reference_histograms_masked(x, m, 0.8)),
    "HM.transform_masked": (ALL, False, True, lambda x, last, m: [H(DEV).transform_masked(x, HIST, m, 0.8, per_tile=p, return_tables=p) for p in (False, True)]),
    "HM.estimate_histograms": (ALL, True, True, lambda x, last, m: [H(DEV, channel_axis=-1 if last else 1).estimate_histograms(x, per_tile=p, masked=k, mask=m) for p in (False, True) for k in (False, True)]),
    "HM.lookup_tables": ((U8,), False, False, lambda x, last, m: H(DEV).lookup_tables(torch.ones(2, 3, 256, dtype=torch.int64), torch.full((2,), 256), HIST)),
    "HM.apply_tables": (ALL, True, False, lambda x, last, m: [H(DEV, channel_axis=-1 if last else 1).apply_tables(x, t) for t in (TABLES[0], TABLES.expand(n_of(x), 3, 256))]),
    "HM.apply_tables_masked": (ALL, False, True, lambda x, last, m: H(DEV).apply_tables_masked(x, TABLES, m, 0.8)),
    "HM.local_counts + apply_with_counts": (ALL, True, False, lambda x, last, m: then(H(DEV, channel_axis=-1 if last else 1), lambda be: be.apply_with_counts(x, be.local_counts(x), 2 * 48 * 48, HIST))),
    "HM(diag).transform": ((U8,), False, False, lambda x, last, m: H(DEV, diag=True).transform(x, HIST)),
    "tissue_mask_native": (ALL, True, False, lambda x, last, m: B.tissue_mask_native(x, 0.8, last)),
    "luminosity_histogram_native": (ALL, True, False, lambda x, last, m: [B.luminosity_histogram_native(x, p, last) for p in (False, True)]),
    "tissue_mask_tiles_native": (ALL, True, False, lambda x, last, m: B.tissue_mask_tiles_native(x, torch.full((n_of(x),), 0.7, dtype=torch.float64), last)),
    "mask_morphology_native": ((U8,), False, False, lambda x, last, m: [B.mask_morphology_native(mask_of(x, False), op, 2, e) for op in ("erode", "dilate", "open", "close") for e in ("square", "disk")]),
    "mask_components_native": ((U8,), False, False, lambda x, last, m: [B.mask_components_native(mask_of(x, False).bool(), c, h) for c in (4, 8) for h in (False, True)]),
    "mask_area_filter_native": ((U8,), False, False, lambda x, last, m: B.mask_area_filter_native(mask_of(x, False), 5, 8, False)),
    "saturation_map_native": (ALL, True, False, lambda x, last, m: B.saturation_map_native(x, last)),
    "median_filter_native": ((U8,), False, False, lambda x, last, m: B.median_filter_native(x[:, 0].contiguous(), 3)),
    "level_histogram_native": ((U8,), False, False, lambda x, last, m: [B.level_histogram_native(x[:, 0].contiguous(), p) for p in (False, True)]),
    "level_mask_native": ((U8,), False, False, lambda x, last, m: B.level_mask_native(x[:, 0].contiguous(), torch.full((n_of(x),), 128, dtype=torch.int32, device=DEV))),
    "sample_pixels_native": (ALL, True, True, lambda x, last, m: [B.sample_pixels_native(x, m, 4, 8, p, 3, last) for p in (False, True)]),
}
X8, XF = batch(U8), batch(F32)
REFUSED = {      # one fault each
    "transform: stain_matrix (2, 3)": lambda: M(DEV).transform(X8, FIT[0].t(), FIT[1]),
    "transform: target_max_conc of 3": lambda: M(DEV).transform(X8, FIT[0], torch.ones(3)),
    "transform: float32 -> bfloat16": lambda: M(DEV).transform(XF, *FIT, out_dtype=BF16),
    "transform: int32 images": lambda: M(DEV).transform(X8.int(), *FIT),
    "transform: NHWC taken as NCHW": lambda: M(DEV).transform(batch(U8, True), *FIT),
    "augment: one of the pair": lambda: M(DEV).augment(X8, rows(2, 2, 1), rows(2, 2, 2), FIT[0]),
    "augment: alpha (1, 2)": lambda: M(DEV).augment(X8, rows(1, 2, 1), rows(2, 2, 2)),
    "separate: nothing asked for": lambda: M(DEV).separate(X8, stains=False),
    "estimate: sampled": lambda: M(DEV, precision="sampled").estimate(X8),
    "apply: source_he (3, 3, 2)": lambda: M(DEV).apply(X8, torch.ones(3, 3, 2), torch.ones(3, 2), *FIT),
    "apply: own basis without factors": lambda: M(DEV).apply(X8, *source(X8, 1)),
    "apply: no source_max_c": lambda: M(DEV).apply(X8, source(X8, 1)[0], N, *FIT),
    "transform_masked: mask (2, 48, 47)": lambda: M(DEV).transform_masked(X8, *FIT, torch.ones(2, 48, 47, dtype=U8)),
    "transform_masked: float mask": lambda: M(DEV).transform_masked(X8, *FIT, torch.ones(2, 48, 48)),
    "separate_apply_masked: sampled": lambda: M(DEV, precision="sampled").separate_apply_masked(X8, *source(X8, 1), *FIT, N),
    "vahadane_estimate: 3 inits": lambda: V(DEV).vahadane_estimate(X8, torch.ones(3, 3, 2)),
    "luminosity apply: 3 rows": lambda: L(DEV).apply(X8, torch.ones(3)),
    "deconv apply: basis (3, 2)": lambda: D(DEV).apply(X8, HED[:, :2]),
    "deconv apply: alpha alone": lambda: D(DEV).apply(X8, HED, alpha=rows(2, 3, 1)),
    "deconv apply: masked NHWC": lambda: D(DEV).apply(batch(U8, True), HED, channels_last=True, masking=(N, 0.8)),
    "deconv apply: mask (1, 48, 48)": lambda: D(DEV).apply(X8, HED, masking=(torch.ones(1, 48, 48, dtype=U8), 0.8)),
    "deconv combine: uint8 / 255": lambda: D(DEV).combine(XF, HED, normalize_to_0_1=True),
    "deconv quantify: bin_log2 9": lambda: D(DEV).quantify(X8, HED, bin_log2=9),
    "reinhard transform: 4 channels": lambda: R(DEV).transform(torch.zeros(2, 4, 8, 8, dtype=U8), *LAB),
    "reinhard transform: mean of 2": lambda: R(DEV).transform(X8, LAB[0][:2], LAB[1]),
    "reinhard apply_statistics: 3 rows": lambda: R(DEV).apply_statistics(X8, LAB[0].expand(3, 3), LAB[1].expand(3, 3), *LAB),
    "reinhard apply_targets: 3 rows": lambda: R(DEV).apply_targets(X8, *LAB, LAB[0].expand(3, 3), LAB[1].expand(3, 3)),
    "reinhard apply_statistics_masked: rows differ": lambda: R(DEV).apply_statistics_masked(X8, LAB[0], LAB[1].expand(2, 3), *LAB, N, 0.8),
    "hm transform: 3-D": lambda: H(DEV).transform(X8[0], HIST),
    "hm transform: NCHW with channel_axis -1": lambda: H(DEV, channel_axis=-1).transform(X8, HIST),
    "hm transform: empty reference list": lambda: H(DEV).transform(X8, []),
    "hm lookup_tables: counts (3, 256)": lambda: H(DEV).lookup_tables(torch.ones(3, 256), torch.ones(1), HIST),
    "hm apply_tables: float64 tables": lambda: H(DEV).apply_tables(X8, TABLES.double()),
    "hm apply_with_counts: no pixels (refused by the library)": lambda: H(DEV).apply_with_counts(X8, torch.ones(3, 256, dtype=torch.int64), 0, HIST),
    "hm(diag) apply_with_counts: no pixels (refused by the diagnostic library)": lambda: (_native.require().sx_hm_tables(N, N, 0, N, N, N), H(DEV, diag=True).apply_with_counts(X8, torch.ones(3, 256, dtype=torch.int64), 0, HIST)),
    "mask_morphology_native: CPU mask": lambda: B.mask_morphology_native(torch.ones(2, 8, 8, dtype=U8), "erode", 1, "square"),
}


def record(label, fn):
    del LOG[:]
    entry = {"call": label}
    try:
        entry["returns"] = describe(fn())
    except Exception as exc:      # noqa: BLE001 -- the refusal IS the record
        entry["raises"] = f"{type(exc).__name__}: {exc}"
    torch.cuda.synchronize()
    entry["trace"] = list(LOG)
    return entry


def digest(entries):
    """The calls in short: per method (all its dtypes, layouts, masks and empty batches together) the number of calls, the library's
    entry points they reached and one sha256 over their full traces and what came back; a refused call is its refusal in full."""
    groups: dict = {}
    for entry in entries:
        groups.setdefault(entry["call"].split(" | ")[0] if not entry["call"].startswith("refused") else entry["call"], []).append(entry)
    short = []
    for label, group in groups.items():
        row = {"call": label, "calls": len(group), "entry_points": " ".join(sorted({t[0][3:] for e in group for t in e["trace"]})),
               "sha256": hashlib.sha256(json.dumps(group, sort_keys=True).encode()).hexdigest()}
        if label.startswith("refused"):
            row = {"call": label, "raises": group[0].get("raises"), "sha256": row["sha256"]}
        short.append(row)
    return short


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true", help="every trace and every description in full (large)")
    args = ap.parse_args()
    _native._lib, _native._diag_lib = Recorder(_native.require()), Recorder(_native.require_diag())
    entries = []
    for label, (dtypes, nhwc, masked, call) in CASES.items():
        runs = [(dt, last, explicit, "full") for dt in dtypes for last in ((False, True) if nhwc else (False,)) for explicit in ((True, False) if masked else (False,))]
        runs += [(dtypes[0], False, masked, "N=0"), (dtypes[0], False, masked, "H=0")]
        for dt, last, explicit, variant in runs:
            x = batch(dt, last, variant)
            m = mask_of(x, last) if explicit else None
            entries.append(record(f"{label} | {str(dt)[6:]} {'NHWC' if last else 'NCHW'} {'explicit mask' if explicit else 'no mask' if not masked else 'mask=None'} {variant}",
                                  lambda: call(x, last, m)))
    entries += [record(f"refused | {label}", fn) for label, fn in REFUSED.items()]
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in (entries if args.full else digest(entries))) + "\n]\n")
    print(f"{len(entries)} calls recorded, {sum('raises' in e for e in entries)} of them raised -> {args.out}")


if __name__ == "__main__":
    main()
