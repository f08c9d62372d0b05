"""Fingerprint of what a build of the library answers on its host side, for comparing two builds (a refactor against its parent).
    python tools/host_layer_fingerprint.py LIB.so --part cpu --out FILE.json     # sizes, forms, refused calls: needs NO device, refuses to run with one
    python tools/host_layer_fingerprint.py LIB.so --part gpu --out FILE.json     # sha256 of every output buffer of a list of small calls
The cpu part calls the entry points with made-up pointers: every call in its list is refused before anything is enqueued, and a call
that a build does NOT refuse is recorded as "not refused" by its launch error -- on a machine with a device it would fault it, hence
the refusal.  The file holds a count and a sha256 per group of records (--full: every record).  Two builds of the same behaviour give
byte-identical files.  Evidence for a change, not a test: nothing is asserted."""
import argparse, hashlib, itertools, json, sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from stainx_amd import _native, synth

NORM, NHWC, SAMPLED, NO_TIE, CLASSIC, OUT_BF16, OUT_F16, SPEC_FAIL, TWO_PASS, FUSE, RESIDENT, NO_CODES = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048
DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64]
SX_ERR_LAUNCH = 4      # include/stainx_hip.h


def is_diag(lib):
    return hasattr(lib, "sx_hm_workspace_parity_offset")


# ---- cpu part -------------------------------------------------------------------------------------------------------------------
P, W, BIG = 0x100000, 0x200000, 1 << 44      # made-up device pointers (W: 256-byte aligned) and a workspace size that is always enough
DEFAULTS = dict(images=P, out=P, dtype=3, n=2, h=48, w=48, sm=P, tmc=P, flags=0, ws=W, ws_bytes=BIG, stream=None, alpha=P, beta=P, stains=P, conc=P, tile_he=P, tile_maxc=P,
                tile_tissue=P, src_he=P, src_maxc=P, n_sources=1, he_out=P, maxc_out=P, mask=P, pooled=0, kept=P, counts=P, basis=P, n_bases=1, target=P, n_targets=1, bin_log2=4, zero_bin=8,
                per_tile=0, qout=P, moments=P, sample=P, record=P, stage=0, n_all=1 << 21, sample_count=4096, sums=P)
CALLS = {
    "sx_macenko_transform": "images out dtype n h w sm tmc flags ws ws_bytes stream",
    "sx_macenko_augment": "images out dtype n h w alpha beta sm tmc flags ws ws_bytes stream",
    "sx_macenko_separate": "images stains conc dtype n h w sm tmc tile_he tile_maxc flags ws ws_bytes stream",
    "sx_macenko_estimate": "images dtype n h w tile_he tile_maxc tile_tissue flags ws ws_bytes stream",
    "sx_macenko_apply": "images out dtype n h w src_he src_maxc n_sources alpha beta sm tmc flags stream",
    "sx_macenko_fit": "images dtype n h w he_out maxc_out ws ws_bytes stream",
    "sx_macenko_estimate_masked": "images dtype n h w mask pooled he_out maxc_out kept counts flags ws ws_bytes stream",
    "sx_macenko_transform_masked": "images out dtype n h w mask sm tmc flags ws ws_bytes stream",
    "sx_macenko_apply_masked": "images out dtype n h w src_he src_maxc n_sources alpha beta sm tmc mask flags stream",
    "sx_macenko_separate_apply": "images stains conc dtype n h w src_he src_maxc n_sources sm tmc flags stream",
    "sx_macenko_separate_apply_masked": "images stains conc dtype n h w src_he src_maxc n_sources sm tmc mask flags stream",
    "sx_macenko_separate_masked": "images stains conc dtype n h w mask sm tmc tile_he tile_maxc flags ws ws_bytes stream",
    "sx_macenko_augment_masked": "images out dtype n h w mask alpha beta sm tmc flags ws ws_bytes stream",
    "sx_macenko_dfit_moments": "images dtype n h w moments ws ws_bytes stream",
    "sx_macenko_pfit_stats": "images dtype n h w moments sample ws ws_bytes stream",
    "sx_macenko_pfit_stats_packed": "images dtype n h w record ws ws_bytes stream",
    "sx_macenko_pfit_pass": "images dtype n h w stage n_all sample_count sums ws ws_bytes stream",
    "sx_deconv_apply": "images out dtype n h w basis n_bases target n_targets alpha beta flags stream",
    "sx_deconv_apply_masked": "images out dtype n h w basis n_bases target n_targets alpha beta mask flags stream",
    "sx_deconv_separate": "images stains conc dtype n h w basis n_bases flags stream",
    "sx_deconv_combine": "conc out dtype n h w basis n_bases flags stream",
    "sx_deconv_quantify": "images dtype n h w basis n_bases bin_log2 zero_bin per_tile qout flags stream",
    "sx_deconv_quantify_masked": "images dtype n h w basis n_bases bin_log2 zero_bin per_tile qout mask flags stream",
    # the Reinhard and histogram-matching host layer, sx_tissue_mask, sx_luminosity_apply
    "sx_reinhard_fit": "images dtype n h w mean_out std_out ws ws_bytes stream",
    "sx_reinhard_transform": "images out dtype n h w ref_mean ref_std ws ws_bytes stream",
    "sx_reinhard_transform_ready": "images out dtype n h w ref_mean ref_std ws ws_bytes stream",
    "sx_reinhard_sums": "images dtype n h w sums ws ws_bytes stream",
    "sx_reinhard_apply": "images out dtype n h w sums n_total ref_mean ref_std ws ws_bytes stream",
    "sx_reinhard_tile_stats": "images dtype n h w mean_out std_out ws ws_bytes stream",
    "sx_reinhard_transform_tiles": "images out dtype n h w ref_mean ref_std mean_out std_out ws ws_bytes stream",
    "sx_reinhard_apply_stats": "images out dtype n h w src_mean src_std n_sources ref_mean ref_std stream",
    "sx_reinhard_stats_masked": "images dtype n h w mask threshold per_tile mean_out std_out counts ws ws_bytes stream",
    "sx_reinhard_transform_masked": "images out dtype n h w ref_mean ref_std mask threshold per_tile mean_out std_out counts ws ws_bytes stream",
    "sx_reinhard_apply_stats_masked": "images out dtype n h w src_mean src_std n_sources ref_mean ref_std mask threshold stream",
    "sx_reinhard_apply_targets": "images out dtype n h w src_mean src_std n_sources tgt_mean tgt_std n_targets stream",
    "sx_reinhard_apply_targets_masked": "images out dtype n h w src_mean src_std n_sources tgt_mean tgt_std n_targets mask threshold stream",
    "sx_hm_fit": "images dtype n h w channels_last hist ws ws_bytes stream",
    "sx_hm_transform": "images out dtype n h w channels_last ref_hist ws ws_bytes stream",
    "sx_hm_fit_ready": "images dtype n h w channels_last hist ws ws_bytes stream",
    "sx_hm_transform_ready": "images out dtype n h w channels_last ref_hist ws ws_bytes stream",
    "sx_hm_counts_ready": "images dtype n h w channels_last counts ws ws_bytes stream",
    "sx_hm_counts": "images dtype n h w channels_last counts ws ws_bytes stream",
    "sx_hm_apply": "images out dtype n h w channels_last counts n_total ref_hist ws ws_bytes stream",
    "sx_hm_transform_tiles": "images out dtype n h w channels_last ref_hist tile_counts lut ws ws_bytes stream",
    "sx_hm_fit_masked": "images dtype n h w channels_last mask threshold hist tissue_out ws ws_bytes stream",
    "sx_hm_transform_masked": "images out dtype n h w channels_last ref_hist mask threshold per_tile tile_counts lut tissue_out ws ws_bytes stream",
    "sx_hm_estimate": "images dtype n h w channels_last per_tile counts pixels_out ws ws_bytes stream",
    "sx_hm_estimate_masked": "images dtype n h w channels_last per_tile mask threshold counts pixels_out ws ws_bytes stream",
    "sx_hm_apply_tables": "images out dtype n h w channels_last lut n_sources stream",
    "sx_hm_apply_tables_masked": "images out dtype n h w channels_last lut n_sources mask threshold stream",
    "sx_tissue_mask": "images dtype n h w channels_last threshold mask_out counts stream",
    "sx_luminosity_apply": "images out2 dtype n h w luminance n_sources stream",
}
DEFAULTS.update(dict(mean_out=P, std_out=P, ref_mean=P, ref_std=P, src_mean=P, src_std=P, tgt_mean=P, tgt_std=P, hist=P, ref_hist=P, tile_counts=P, lut=P, tissue_out=P, pixels_out=P,
                     mask_out=P, luminance=P, out2=P + 0x100000, n_total=4608.0, threshold=0.8, channels_last=0))
POINTERS = {k for k, v in DEFAULTS.items() if v == P} | {"ws", "out2"}
# two faults in one call: which of the two an entry point reports is the order of its checks
PAIRS = [dict(dtype=7, ws_bytes=0), dict(dtype=7, n=0), dict(images=None, ws_bytes=0), dict(n_sources=3, dtype=7), dict(n_targets=3, dtype=7), dict(n=0, ws_bytes=0), dict(n=1 << 25, dtype=7),
         dict(n=1 << 25, ws_bytes=0), dict(mask=None, threshold=1.5, dtype=7), dict(mask=None, threshold=1.5, ws_bytes=0), dict(mask=None, threshold=1.5, n=0), dict(mask=None, threshold=1.5, n_sources=3),
         dict(mask=None, threshold=1.5, n=1 << 25), dict(n_sources=3, n=0), dict(n_sources=3, n_targets=3), dict(dtype=7, ws=W + 8), dict(out2=P, dtype=7), dict(out2=P, n_sources=3),
         dict(n_total=0.5, dtype=7), dict(n_total=0.5, images=None), dict(mean_out=None, images=None), dict(ref_mean=None, images=None), dict(counts=None, images=None), dict(lut=None, n=0),
         dict(mask_out=None, counts=None), dict(mask_out=None, counts=None, images=None)]


def mutations(params):
    """(label, overrides) of every refused variant of one entry point."""
    ptrs = [p for p in params if p in POINTERS]
    for p in ptrs:
        yield f"{p}=null", {p: None}
    for a, b in (("stains", "conc"), ("sm", "tmc"), ("alpha", "beta")):
        if a in params and b in params:
            yield f"{a}={b}=null", {a: None, b: None}
    if {"sm", "alpha"} <= set(params):
        yield "sm=tmc=alpha=beta=null", dict(sm=None, tmc=None, alpha=None, beta=None)
    for label, o in (("n=0", dict(n=0)), ("h=-1", dict(h=-1)), ("w=0", dict(w=0)), ("2^32 pixels", dict(n=1 << 20, h=64, w=64)), ("dtype=7", dict(dtype=7))):
        yield label, o
    if "ws" in params:
        yield "ws_bytes=0", dict(ws_bytes=0)
        yield "ws_bytes=4096", dict(ws_bytes=4096)
        yield "ws misaligned", dict(ws=W + 8)
    if "flags" in params:
        for bit in range(12):
            for dt in (0, 3):
                yield f"flags={1 << bit} dtype={dt}", dict(flags=1 << bit, dtype=dt)
        for dt in (0, 3):
            yield f"flags=both OUT dtype={dt}", dict(flags=OUT_BF16 | OUT_F16, dtype=dt)
            yield f"flags=OUT_F16|NHWC dtype={dt}", dict(flags=OUT_F16 | NHWC, dtype=dt)
    for k in ("n_sources", "n_bases", "n_targets"):
        if k in params:
            yield f"{k}=3", {k: 3}
    if "bin_log2" in params:
        yield "bin_log2=9", dict(bin_log2=9)
        yield "zero_bin=256", dict(zero_bin=256)
    if "stage" in params:
        yield "stage=2", dict(stage=2)
    for o in (dict(threshold=1.5), dict(threshold=0.0), dict(mask=None, threshold=1.5), dict(mask=None, threshold=0.0), dict(n_total=0.5), dict(channels_last=1), dict(per_tile=1), dict(out2=P),
              dict(n=1 << 25), dict(n=4097, h=8, w=8), *PAIRS):
        yield " ".join(f"{k}={'null' if v is None else v}" for k, v in o.items()), o


def cpu_part(lib):
    diag = is_diag(lib)
    res = {"diag": diag}
    tiles = [(16, 16), (47, 49), (48, 48), (128, 128), (224, 224), (512, 512), (724, 724), (1024, 1024), (2048, 2048)]
    flag_sets = [0, CLASSIC, NHWC, SAMPLED] + ([TWO_PASS, FUSE | TWO_PASS, FUSE, RESIDENT] if diag else [])
    sizes = []
    for n, (h, w) in itertools.product([1, 2, 16, 64, 256, 0, -1], tiles):
        row = {"n": n, "h": h, "w": w, "macenko": lib.sx_macenko_workspace_bytes(n, h, w), "reinhard": lib.sx_reinhard_workspace_bytes(n, h, w), "hm": lib.sx_hm_workspace_bytes(n, h, w),
               "hm_tiles": lib.sx_hm_tiles_workspace_bytes(n, h, w), "hm_masked": lib.sx_hm_masked_workspace_bytes(n, h, w), "sample": lib.sx_sample_workspace_bytes(n, h, w),
               "components": lib.sx_mask_components_workspace_bytes(n, h, w), "pfit_sample_count": lib.sx_macenko_pfit_sample_count(n, h, w), "by_dtype": []}
        for dt in range(5):
            row["by_dtype"].append({"for": [lib.sx_macenko_workspace_bytes_for(dt, n, h, w, f) for f in flag_sets], "form": [lib.sx_macenko_form(dt, n, h, w, f) for f in flag_sets],
                                    "two_pass": [lib.sx_macenko_takes_two_pass(dt, n, h, w, f) for f in flag_sets], "reinhard_for": lib.sx_reinhard_workspace_bytes_for(dt, n, h, w),
                                    "reinhard_tiles": lib.sx_reinhard_tiles_workspace_bytes(dt, n, h, w), "reinhard_masked": lib.sx_reinhard_masked_workspace_bytes(dt, n, h, w),
                                    "vahadane": lib.sx_vahadane_workspace_bytes(dt, n, h, w), "luminosity": lib.sx_luminosity_workspace_bytes(dt, n, h, w)})
        sizes.append(row)
    res["flag_sets"] = flag_sets
    res["sizes"] = sizes
    res["constants"] = {"telemetry_offset": lib.sx_macenko_telemetry_offset(), "dfit_state_bytes": lib.sx_macenko_dfit_state_bytes()}
    refused, not_refused = [], []
    for name, spec in CALLS.items():
        params = spec.split()
        fn = getattr(lib, name)
        seen = set()
        for label, o in mutations(params):
            if not o or label in seen or not set(o) <= set(params):
                continue
            seen.add(label)
            args = {**DEFAULTS, **o}
            rc = fn(*[args[p] for p in params])
            if rc == 0 or rc == SX_ERR_LAUNCH:      # (a nullable pointer, a flag this build takes: the call went on to launch -- on nothing)
                not_refused.append([name, label])
            else:
                refused.append([name, label, rc, _native.last_error(lib)])
    res["refused"] = refused
    res["not_refused"] = not_refused
    return res


# ---- gpu part -------------------------------------------------------------------------------------------------------------------
def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


class Gpu:
    def __init__(self, lib):
        self.lib, self.dev = lib, torch.device("cuda:0")
        self.out, self.batches = {}, {}
        he = [[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]]      # (torchstain's default reference)
        self.sm = torch.tensor(he, dtype=torch.float32, device=self.dev).contiguous()
        self.tmc = torch.tensor([1.9705, 1.0308], dtype=torch.float32, device=self.dev).contiguous()
        self.src_he = (self.sm * 1.03).contiguous()
        self.src_maxc = (self.tmc * 0.9).contiguous()
        hed = torch.tensor([[0.65, 0.07, 0.27], [0.70, 0.99, 0.57], [0.29, 0.11, 0.78]], dtype=torch.float32)
        self.basis = hed.to(self.dev).contiguous()

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def images(self, n, h, w, dtype, nhwc, offset):
        if (n, h, w) not in self.batches:      # (more than 16 tiles: the first 16, shifted by a column more per repeat)
            base = synth.he_batch(min(n, 16), h, w, seed0=4100 + h, scale_step=0.05)
            self.batches[(n, h, w)] = base if n <= 16 else torch.cat([base.roll(k, dims=-1) for k in range((n + 15) // 16)])[:n]
        x = synth.as_dtype(self.batches[(n, h, w)], dtype)
        if nhwc:
            x = x.permute(0, 2, 3, 1).contiguous()
        flat = torch.zeros(x.numel() + 16, dtype=dtype, device=self.dev)      # (offset: a view one element in -> the scalar path by pointer)
        view = flat[offset:offset + x.numel()]
        view.copy_(x.reshape(-1).to(self.dev))
        return view

    def mask(self, n, h, w, kind, offset=0):
        m = torch.ones(n, h, w, dtype=torch.uint8)
        if kind == "half":
            m[:, :, : w // 2] = 0
        flat = torch.zeros(m.numel() + 16, dtype=torch.uint8, device=self.dev)
        view = flat[offset:offset + m.numel()]
        view.copy_(m.reshape(-1).to(self.dev))
        return view

    def factors(self, n, k):
        a = torch.linspace(0.8, 1.2, n * k, dtype=torch.float32).reshape(n, k).to(self.dev).contiguous()
        b = torch.linspace(-0.05, 0.05, n * k, dtype=torch.float32).reshape(n, k).to(self.dev).contiguous()
        return a, b

    def out_dtype(self, dtype, flags):
        if dtype == torch.uint8:
            return torch.bfloat16 if flags & OUT_BF16 else torch.float16 if flags & OUT_F16 else torch.float32 if flags & NORM else torch.uint8
        return dtype

    def workspace(self, n, h, w):
        return torch.zeros(max(self.lib.sx_macenko_workspace_bytes(n, h, w), 256), dtype=torch.uint8, device=self.dev)

    def record(self, key, rc, *tensors):
        torch.cuda.synchronize()
        self.out[key] = {"rc": rc, "sha256": digest(*tensors)} if rc == 0 else {"rc": rc, "error": _native.last_error(self.lib)}

    def run(self, call, key, dtype, n, h, w, flags, offset=0, mask_kind=None, mask_offset=0, variant=""):
        lib, code = self.lib, _native.DTYPE_CODES[dtype]
        nhwc = bool(flags & NHWC)
        x = self.images(n, h, w, dtype, nhwc, offset)
        od = self.out_dtype(dtype, flags)
        px = n * h * w
        z = lambda count, dt=torch.float32: torch.zeros(count, dtype=dt, device=self.dev)
        ws = self.workspace(n, h, w)
        a2, b2 = self.factors(n, 2)
        a3, b3 = self.factors(n, 3)
        m = self.mask(n, h, w, mask_kind, mask_offset) if mask_kind else None
        p, s = self.ptr, None
        if call in ("transform", "augment", "augment_own"):
            out = z(3 * px, od)
            if call == "transform":
                rc = lib.sx_macenko_transform(p(x), p(out), code, n, h, w, p(self.sm), p(self.tmc), flags, p(ws), ws.numel(), s)
            else:
                sm, tmc = (self.sm, self.tmc) if call == "augment" else (None, None)
                rc = lib.sx_macenko_augment(p(x), p(out), code, n, h, w, p(a2), p(b2), p(sm), p(tmc), flags, p(ws), ws.numel(), s)
            return self.record(key, rc, out)
        if call in ("separate", "separate_apply", "separate_masked", "separate_apply_masked"):
            stains = z(2 * 3 * px, od) if "stains" in variant else None
            conc = z(2 * px) if "conc" in variant else None
            the, tmaxc = z(6 * n), (z(2 * n) if "maxc" in variant else None)
            sm, tmc = (None, None) if "own" in variant else (self.sm, self.tmc)
            if call == "separate":
                rc = lib.sx_macenko_separate(p(x), p(stains), p(conc), code, n, h, w, p(sm), p(tmc), p(the), p(tmaxc), flags, p(ws), ws.numel(), s)
            elif call == "separate_masked":
                rc = lib.sx_macenko_separate_masked(p(x), p(stains), p(conc), code, n, h, w, p(m), p(sm), p(tmc), p(the), p(tmaxc), flags, p(ws), ws.numel(), s)
            elif call == "separate_apply":
                rc = lib.sx_macenko_separate_apply(p(x), p(stains), p(conc), code, n, h, w, p(self.src_he), p(self.src_maxc), 1, p(sm), p(tmc), flags, s)
            else:
                rc = lib.sx_macenko_separate_apply_masked(p(x), p(stains), p(conc), code, n, h, w, p(self.src_he), p(self.src_maxc), 1, p(sm), p(tmc), p(m), flags, s)
            return self.record(key, rc, stains, conc, the, tmaxc)
        if call in ("estimate", "fit", "estimate_masked"):
            he, mc, tis, cnt = z(6 * n), z(2 * n), z(n), z(n, torch.int64)
            if call == "estimate":
                rc = lib.sx_macenko_estimate(p(x), code, n, h, w, p(he), p(mc), p(tis), flags, p(ws), ws.numel(), s)
            elif call == "fit":
                rc = lib.sx_macenko_fit(p(x), code, n, h, w, p(he), p(mc), p(ws), ws.numel(), s)
            else:
                rc = lib.sx_macenko_estimate_masked(p(x), code, n, h, w, p(m), 1 if "pooled" in variant else 0, p(he), p(mc), p(tis), p(cnt), flags, p(ws), ws.numel(), s)
            return self.record(key, rc, he, mc, tis, cnt)
        if call in ("apply", "apply_masked", "transform_masked", "augment_masked"):
            out = z(3 * px, od)
            if call == "apply":
                rc = lib.sx_macenko_apply(p(x), p(out), code, n, h, w, p(self.src_he), p(self.src_maxc), 1, p(a2), p(b2), p(self.sm), p(self.tmc), flags, s)
            elif call == "apply_masked":
                rc = lib.sx_macenko_apply_masked(p(x), p(out), code, n, h, w, p(self.src_he), p(self.src_maxc), 1, p(a2), p(b2), p(self.sm), p(self.tmc), p(m), flags, s)
            elif call == "transform_masked":
                rc = lib.sx_macenko_transform_masked(p(x), p(out), code, n, h, w, p(m), p(self.sm), p(self.tmc), flags, p(ws), ws.numel(), s)
            else:
                rc = lib.sx_macenko_augment_masked(p(x), p(out), code, n, h, w, p(m), p(a2), p(b2), p(self.sm), p(self.tmc), flags, p(ws), ws.numel(), s)
            return self.record(key, rc, out)
        if call in ("deconv_apply", "deconv_apply_masked"):
            out = z(3 * px, od)
            if call == "deconv_apply":
                rc = lib.sx_deconv_apply(p(x), p(out), code, n, h, w, p(self.basis), 1, None, 1, p(a3), p(b3), flags, s)
            else:
                rc = lib.sx_deconv_apply_masked(p(x), p(out), code, n, h, w, p(self.basis), 1, None, 1, p(a3), p(b3), p(m), flags, s)
            return self.record(key, rc, out)
        if call == "deconv_separate":
            stains = z(3 * 3 * px, od) if "stains" in variant else None
            conc = z(3 * px) if "conc" in variant else None
            rc = lib.sx_deconv_separate(p(x), p(stains), p(conc), code, n, h, w, p(self.basis), 1, flags, s)
            return self.record(key, rc, stains, conc)
        if call == "deconv_combine":      # (dtype: the output's; the concentrations: a separation of the uint8 batch)
            u8 = self.images(n, h, w, torch.uint8, nhwc, 0)
            tmp, conc = z(3 * px), z(3 * px + 4)[offset:offset + 3 * px]      # (offset: the concentrations one element in)
            rc = lib.sx_deconv_separate(p(u8), None, p(tmp), 0, n, h, w, p(self.basis), 1, flags & NHWC, s)
            conc.copy_(tmp)
            out = z(3 * px, dtype)
            rc = rc or lib.sx_deconv_combine(p(conc), p(out), code, n, h, w, p(self.basis), 1, flags, s)
            return self.record(key, rc, out)
        if call in ("deconv_quantify", "deconv_quantify_masked"):
            rows = n if "per_tile" in variant else 1
            out = z(rows * 772, torch.int64)
            if call == "deconv_quantify":
                rc = lib.sx_deconv_quantify(p(x), code, n, h, w, p(self.basis), 1, 5, 64, rows != 1, p(out), flags, s)
            else:
                rc = lib.sx_deconv_quantify_masked(p(x), code, n, h, w, p(self.basis), 1, 5, 64, rows != 1, p(out), p(m), flags, s)
            return self.record(key, rc, out)
        raise ValueError(call)


def siblings(g, tag, dtype, n, h, w, offset=0, out_offset=0, masks=("half", "ones", "rule"), mask_offset=0, reinhard_bytes=None, only=None):
    """Every Reinhard / histogram-matching / tissue-mask / luminosity-apply entry point on one batch: records `<entry point> <tag> ...`.
    Workspaces are zero-filled per call (the READY state); reinhard_bytes: the Reinhard workspace's size instead of the largest query."""
    lib, dev, code, p, s = g.lib, g.dev, _native.DTYPE_CODES[dtype], g.ptr, None
    px, rows = n * h * w, torch.arange(n * 3, dtype=torch.float32, device=dev)
    z = lambda count, dt=torch.float32: torch.zeros(count, dtype=dt, device=dev)
    img_out = lambda: z(3 * px + 16, dtype)[out_offset:out_offset + 3 * px]
    want = lambda name: only is None or name in only
    ref_mean, ref_std = torch.tensor([0.62, 0.11, -0.04], device=dev), torch.tensor([0.17, 0.08, 0.05], device=dev)
    tgt_mean, tgt_std = (0.55 + 0.01 * rows).contiguous(), (0.12 + 0.002 * rows).contiguous()
    src_mean, src_std = (0.60 - 0.01 * rows).contiguous(), (0.15 + 0.001 * rows).contiguous()
    ref_hist = torch.linspace(1.0, 2.0, 768, device=dev).reshape(3, 256)
    ref_hist = (ref_hist / ref_hist.sum(dim=1, keepdim=True)).contiguous()

    def mask_of(kind):      # (pointer or None, threshold)
        return (None, 0.8) if kind == "rule" else (g.mask(n, h, w, kind, mask_offset), 0.0)

    # ---- Reinhard (planar only)
    x = g.images(n, h, w, dtype, False, offset)
    rb = reinhard_bytes or max(lib.sx_reinhard_workspace_bytes_for(code, n, h, w), lib.sx_reinhard_tiles_workspace_bytes(code, n, h, w), lib.sx_reinhard_masked_workspace_bytes(code, n, h, w))
    ws = lambda: z(rb, torch.uint8)
    status = lambda wsp: wsp[lib.sx_reinhard_workspace_status_offset():][:4]
    if want("reinhard_pooled"):
        m, sd, wsp = z(3), z(3), ws()
        g.record(f"sx_reinhard_fit {tag}", lib.sx_reinhard_fit(p(x), code, n, h, w, p(m), p(sd), p(wsp), rb, s), m, sd)
        for name in ("sx_reinhard_transform", "sx_reinhard_transform_ready"):
            out, wsp = img_out(), ws()
            g.record(f"{name} {tag}", getattr(lib, name)(p(x), p(out), code, n, h, w, p(ref_mean), p(ref_std), p(wsp), rb, s), out, status(wsp))
        sums, out, wsp = z(6, torch.float64), img_out(), ws()
        rc = lib.sx_reinhard_sums(p(x), code, n, h, w, p(sums), p(wsp), rb, s)
        rc = rc or lib.sx_reinhard_apply(p(x), p(out), code, n, h, w, p(sums), float(px), p(ref_mean), p(ref_std), p(wsp), rb, s)
        g.record(f"sx_reinhard_sums+apply {tag}", rc, sums, out)
    if want("reinhard_tiles"):
        tm, ts, wsp = z(3 * n), z(3 * n), ws()
        g.record(f"sx_reinhard_tile_stats {tag}", lib.sx_reinhard_tile_stats(p(x), code, n, h, w, p(tm), p(ts), p(wsp), rb, s), tm, ts)
        for given in (True, False):
            out, m, sd, wsp = img_out(), z(3 * n) if given else None, z(3 * n) if given else None, ws()
            g.record(f"sx_reinhard_transform_tiles {tag} stats_out={given}", lib.sx_reinhard_transform_tiles(p(x), p(out), code, n, h, w, p(ref_mean), p(ref_std), p(m), p(sd), p(wsp), rb, s), out, m, sd)
    if want("reinhard_given"):
        for ns in sorted({1, n}):
            out = img_out()
            g.record(f"sx_reinhard_apply_stats {tag} n_sources={ns}", lib.sx_reinhard_apply_stats(p(x), p(out), code, n, h, w, p(src_mean), p(src_std), ns, p(ref_mean), p(ref_std), s), out)
            out = img_out()
            g.record(f"sx_reinhard_apply_targets {tag} n_sources=n_targets={ns}", lib.sx_reinhard_apply_targets(p(x), p(out), code, n, h, w, p(src_mean), p(src_std), ns, p(tgt_mean), p(tgt_std), ns, s), out)
        lum = (0.85 + 0.01 * rows[:n]).contiguous()
        for ns in sorted({1, n}):
            out = img_out()
            g.record(f"sx_luminosity_apply {tag} n_sources={ns}", lib.sx_luminosity_apply(p(x), p(out), code, n, h, w, p(lum), ns, s), out)
    for mk in masks:
        mp, thr = mask_of(mk)
        mtag = f"{tag} mask={mk}" + (f"+{mask_offset}" if mask_offset and mk != "rule" else "")
        if want("reinhard_masked"):
            for per_tile in (0, 1):
                k = n if per_tile else 1
                m, sd, cnt, wsp = z(3 * k), z(3 * k), z(k, torch.int64), ws()
                g.record(f"sx_reinhard_stats_masked {mtag} per_tile={per_tile}", lib.sx_reinhard_stats_masked(p(x), code, n, h, w, p(mp), thr, per_tile, p(m), p(sd), p(cnt), p(wsp), rb, s), m, sd, cnt)
                out, cnt, wsp = img_out(), z(k, torch.int64), ws()
                g.record(f"sx_reinhard_transform_masked {mtag} per_tile={per_tile}",
                         lib.sx_reinhard_transform_masked(p(x), p(out), code, n, h, w, p(ref_mean), p(ref_std), p(mp), thr, per_tile, None, None, p(cnt), p(wsp), rb, s), out, cnt)
            out = img_out()
            g.record(f"sx_reinhard_apply_stats_masked {mtag}", lib.sx_reinhard_apply_stats_masked(p(x), p(out), code, n, h, w, p(src_mean), p(src_std), n, p(ref_mean), p(ref_std), p(mp), thr, s), out)
            out = img_out()
            g.record(f"sx_reinhard_apply_targets_masked {mtag}", lib.sx_reinhard_apply_targets_masked(p(x), p(out), code, n, h, w, p(src_mean), p(src_std), n, p(tgt_mean), p(tgt_std), n, p(mp), thr, s), out)
    # ---- histogram matching and the tissue rule, both layouts
    hb = lib.sx_hm_masked_workspace_bytes(n, h, w)
    for cl in (0, 1):
        x = g.images(n, h, w, dtype, bool(cl), offset)
        ltag = f"{tag} channels_last={cl}"
        hws = lambda ready=False: z(hb, torch.uint8)
        hstatus = lambda wsp: wsp[lib.sx_hm_workspace_status_offset():][:4]
        if want("hm_pooled"):
            for name, ready in (("sx_hm_fit", False), ("sx_hm_fit_ready", True)):
                hist, wsp = z(768), hws(ready)
                g.record(f"{name} {ltag}", getattr(lib, name)(p(x), code, n, h, w, cl, p(hist), p(wsp), hb, s), hist, hstatus(wsp))
            for name, ready in (("sx_hm_transform", False), ("sx_hm_transform_ready", True)):
                out, wsp = img_out(), hws(ready)
                g.record(f"{name} {ltag}", getattr(lib, name)(p(x), p(out), code, n, h, w, cl, p(ref_hist), p(wsp), hb, s), out, hstatus(wsp))
            cnt, wsp = z(768, torch.int64), hws(True)
            g.record(f"sx_hm_counts_ready {ltag}", lib.sx_hm_counts_ready(p(x), code, n, h, w, cl, p(cnt), p(wsp), hb, s), cnt, hstatus(wsp))
            cnt, out, wsp = z(768, torch.int64), img_out(), hws()
            rc = lib.sx_hm_counts(p(x), code, n, h, w, cl, p(cnt), p(wsp), hb, s)
            rc = rc or lib.sx_hm_apply(p(x), p(out), code, n, h, w, cl, p(cnt), float(px), p(ref_hist), p(wsp), hb, s)
            g.record(f"sx_hm_counts+apply {ltag}", rc, cnt, out)
        if want("hm_tiles"):
            out, cnt, lut, wsp = img_out(), z(n * 768, torch.int32), z(n * 768), hws()
            g.record(f"sx_hm_transform_tiles {ltag}", lib.sx_hm_transform_tiles(p(x), p(out), code, n, h, w, cl, p(ref_hist), p(cnt), p(lut), p(wsp), hb, s), out, cnt, lut, hstatus(wsp))
            for per_tile in (0, 1):
                k = n if per_tile else 1
                cnt, pix, lut, wsp = z(k * 768, torch.int64), z(k, torch.int64), z(k * 768), hws()
                rc = lib.sx_hm_estimate(p(x), code, n, h, w, cl, per_tile, p(cnt), p(pix), p(wsp), hb, s)
                g.record(f"sx_hm_estimate {ltag} per_tile={per_tile}", rc, cnt, pix, hstatus(wsp))
                out = img_out()
                rc = rc or lib.sx_hm_tables(p(cnt), p(pix), k, p(ref_hist), p(lut), s)
                rc = rc or lib.sx_hm_apply_tables(p(x), p(out), code, n, h, w, cl, p(lut), k, s)
                g.record(f"sx_hm_tables+apply_tables {ltag} n_sources={k}", rc, lut, out)
        if want("tissue_mask"):
            mo, cnt = z(px + 16, torch.uint8)[mask_offset:mask_offset + px], z(n, torch.int64)
            g.record(f"sx_tissue_mask {ltag}" + (f" mask_out+{mask_offset}" if mask_offset else ""), lib.sx_tissue_mask(p(x), code, n, h, w, cl, 0.8, p(mo), p(cnt), s), mo, cnt)
        for mk in masks:
            mp, thr = mask_of(mk)
            mtag = f"{ltag} mask={mk}" + (f"+{mask_offset}" if mask_offset and mk != "rule" else "")
            if not want("hm_masked"):
                continue
            hist, tis, wsp = z(768), z(1, torch.int64), hws()
            g.record(f"sx_hm_fit_masked {mtag}", lib.sx_hm_fit_masked(p(x), code, n, h, w, cl, p(mp), thr, p(hist), p(tis), p(wsp), hb, s), hist, tis)
            for per_tile in (0, 1):
                k = n if per_tile else 1
                out, cnt, lut, tis, wsp = img_out(), z(k * 768, torch.int32), z(k * 768), z(k, torch.int64), hws()
                g.record(f"sx_hm_transform_masked {mtag} per_tile={per_tile}",
                         lib.sx_hm_transform_masked(p(x), p(out), code, n, h, w, cl, p(ref_hist), p(mp), thr, per_tile, p(cnt), p(lut), p(tis), p(wsp), hb, s), out, cnt, lut, tis, hstatus(wsp))
                cnt, pix, wsp = z(k * 768, torch.int64), z(k, torch.int64), hws()
                g.record(f"sx_hm_estimate_masked {mtag} per_tile={per_tile}", lib.sx_hm_estimate_masked(p(x), code, n, h, w, cl, per_tile, p(mp), thr, p(cnt), p(pix), p(wsp), hb, s), cnt, pix, hstatus(wsp))
                out = img_out()
                g.record(f"sx_hm_apply_tables_masked {mtag} n_sources={k}", lib.sx_hm_apply_tables_masked(p(x), p(out), code, n, h, w, cl, p(lut), k, p(mp), thr, s), out)


def siblings_part(g):
    for dtype in DTYPES:
        dn = str(dtype).split(".")[-1]
        siblings(g, f"{dn} 2x48x48", dtype, 2, 48, 48)                                       # whole packs for every element type
        siblings(g, f"{dn} 2x47x49", dtype, 2, 47, 49)                                       # no whole packs
        siblings(g, f"{dn} 2x48x48+1", dtype, 2, 48, 48, offset=1)                           # single elements by the images' pointer
        siblings(g, f"{dn} 2x48x48 out+1", dtype, 2, 48, 48, out_offset=1, masks=("half",))  # ... by the output's
        siblings(g, f"{dn} 2x48x48", dtype, 2, 48, 48, masks=("half",), mask_offset=1, only=("reinhard_masked", "hm_masked", "tissue_mask"))      # ... by the mask's
        siblings(g, f"{dn} 2x512x512", dtype, 2, 512, 512, masks=("half",))                  # more than one 65536-element chunk per plane and per tile
    # the Reinhard codes (4 x 512 x 512: exactly 2^20 pixels): with room for them, and on the plain size without
    siblings(g, "float32 4x512x512 coded", torch.float32, 4, 512, 512, masks=(), only=("reinhard_pooled", "reinhard_tiles"))
    siblings(g, "float32 4x512x512 plain size", torch.float32, 4, 512, 512, masks=(), only=("reinhard_pooled",), reinhard_bytes=g.lib.sx_reinhard_workspace_bytes(4, 512, 512))
    for n in (1, 16, 64):      # the steps of sweeps_for()
        siblings(g, f"uint8 {n}x512x512", torch.uint8, n, 512, 512, masks=("half",), only=("reinhard_pooled", "reinhard_tiles", "reinhard_given", "reinhard_masked"))
        g.batches.pop((n, 512, 512), None)
    siblings(g, "uint8 4097x8x8", torch.uint8, 4097, 8, 8, masks=(), only=("reinhard_pooled",))      # beyond kReadyTiles: a READY call runs as a plain one
    siblings(g, "uint8 48x512x512", torch.uint8, 48, 512, 512, masks=(), only=("hm_pooled",))         # the cap of 2048 workgroups
    g.batches.pop((48, 512, 512), None)


def gpu_part(lib):
    g = Gpu(lib)
    siblings_part(g)
    shapes = [("48x48", 48, 48, 0), ("47x49", 47, 49, 0), ("48x48+1", 48, 48, 1)]      # whole packs / scalar by size / scalar by pointer
    def out_flag_sets(dtype):
        return [0, NORM] + ([OUT_BF16, OUT_F16, OUT_BF16 | NORM, OUT_F16 | NORM] if dtype == torch.uint8 else [])
    imaged = [("transform", ""), ("augment", ""), ("augment_own", ""), ("apply", ""), ("deconv_apply", ""), ("separate", "stains"), ("separate", "stains conc maxc"), ("separate", "stains own"),
              ("separate", "stains conc own maxc"), ("separate_apply", "stains conc"), ("separate_apply", "stains own"), ("deconv_separate", "stains"), ("deconv_separate", "stains conc")]
    plain = [("estimate", ""), ("separate", "conc"), ("separate", "conc own maxc"), ("separate_apply", "conc"), ("deconv_separate", "conc"), ("deconv_quantify", ""), ("deconv_quantify", "per_tile")]
    masked_imaged = [("transform_masked", ""), ("apply_masked", ""), ("augment_masked", ""), ("separate_masked", "stains conc maxc"), ("separate_masked", "stains own"),
                     ("separate_apply_masked", "stains conc"), ("deconv_apply_masked", "")]
    masked_plain = [("estimate_masked", ""), ("estimate_masked", "pooled"), ("separate_masked", "conc"), ("separate_apply_masked", "conc"), ("deconv_quantify_masked", "per_tile")]
    for dtype in DTYPES:
        dn = str(dtype).split(".")[-1]
        for sname, h, w, off in shapes:
            for layout in (0, NHWC):
                for call, var in imaged:
                    for f in out_flag_sets(dtype):
                        g.run(call, f"{call}[{var}] {dn} {sname} flags={f | layout}", dtype, 2, h, w, f | layout, off, variant=var)
                for call, var in plain:
                    g.run(call, f"{call}[{var}] {dn} {sname} flags={layout}", dtype, 2, h, w, layout, off, variant=var)
                g.run("deconv_combine", f"deconv_combine {dn} {sname} flags={layout}", dtype, 2, h, w, layout, off)
                if dtype != torch.uint8:
                    g.run("deconv_combine", f"deconv_combine {dn} {sname} flags={layout | NORM}", dtype, 2, h, w, layout | NORM, off)
            g.run("fit", f"fit {dn} {sname}", dtype, 2, h, w, 0, off)
            for mk in ("half", "ones"):
                for call, var in masked_imaged:
                    for f in out_flag_sets(dtype):
                        g.run(call, f"{call}[{var}] {dn} {sname} mask={mk} flags={f}", dtype, 2, h, w, f, off, mask_kind=mk, variant=var)
                for call, var in masked_plain:
                    g.run(call, f"{call}[{var}] {dn} {sname} mask={mk}", dtype, 2, h, w, 0, off, mask_kind=mk, variant=var)
        for call, var in masked_imaged + masked_plain:      # (the mask's say in `vec`: its pointer one byte in)
            g.run(call, f"{call}[{var}] {dn} 48x48 mask=half+1", dtype, 2, 48, 48, 0, 0, mask_kind="half", mask_offset=1, variant=var)
    # rules keyed on the batch size
    for dtype in (torch.float32, torch.uint8):
        dn = str(dtype).split(".")[-1]
        g.run("transform", f"transform {dn} 16x512x512", dtype, 16, 512, 512, 0)
        g.run("transform", f"transform {dn} 16x512x512 CLASSIC", dtype, 16, 512, 512, CLASSIC)
        g.run("transform", f"transform {dn} 1x512x512", dtype, 1, 512, 512, 0)
        g.run("transform_masked", f"transform_masked {dn} 16x512x512", dtype, 16, 512, 512, 0, mask_kind="half")
        g.run("separate", f"separate {dn} 16x512x512", dtype, 16, 512, 512, 0, variant="stains conc maxc")
    for call, var in (("fit", ""), ("estimate", ""), ("separate", "stains conc maxc"), ("augment", "")):
        g.run(call, f"{call} float32 4x512x512", torch.float32, 4, 512, 512, 0, variant=var)
    if is_diag(lib):
        for name, f in (("TWO_PASS", TWO_PASS), ("FUSE", TWO_PASS | FUSE), ("RESIDENT", RESIDENT), ("NO_CODES", NO_CODES | CLASSIC)):
            g.run("transform", f"transform float32 4x256x256 {name}", torch.float32, 4, 256, 256, f)
    return {"diag": is_diag(lib), "cases": len(g.out), "outputs": g.out}


def dumps(res):
    """JSON with one record per line: small enough to keep, and two files that differ show where in a line diff."""
    parts = []
    for key in sorted(res):
        v = res[key]
        if isinstance(v, list) and v and isinstance(v[0], (list, dict)):
            body = "[\n" + ",\n".join(json.dumps(x, sort_keys=True, separators=(",", ":")) for x in v) + "\n]"
        elif isinstance(v, dict) and v and all(isinstance(x, dict) for x in v.values()):
            body = "{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v[k], sort_keys=True, separators=(",", ":")) for k in sorted(v)) + "\n}"
        else:
            body = json.dumps(v, sort_keys=True)
        parts.append(json.dumps(key) + ": " + body)
    return "{\n" + ",\n".join(parts) + "\n}\n"


def summary(res):
    """The records in groups -- one count and one sha256 over the group's records, in order -- so that the file is short enough to keep:
    refused calls and GPU outputs per entry point, sizes per tile size.  Which record of a group differs: --full."""
    def group(records, key_of):
        groups = {}
        for r in records:
            groups.setdefault(key_of(r), []).append(json.dumps(r, sort_keys=True))
        return {k: {"records": len(v), "sha256": hashlib.sha256("\n".join(v).encode()).hexdigest()} for k, v in sorted(groups.items())}
    out = {k: v for k, v in res.items() if k not in ("refused", "not_refused", "sizes", "outputs")}
    if "outputs" in res:
        out["failed"] = sorted(k for k, v in res["outputs"].items() if v["rc"] != 0)
        out["outputs"] = group(sorted(res["outputs"].items()), lambda r: r[0].replace("[", " ").split()[0])
    else:
        refused, passed = group(res["refused"], lambda r: r[0]), group(res["not_refused"], lambda r: r[0])      # (one line per entry point)
        none = {"records": 0, "sha256": ""}
        out["calls"] = {k: {"refused": refused.get(k, none)["records"], "not_refused": passed.get(k, none)["records"],
                            "sha256": hashlib.sha256((refused.get(k, none)["sha256"] + passed.get(k, none)["sha256"]).encode()).hexdigest()} for k in sorted(set(refused) | set(passed))}
        out["sizes"] = group(res["sizes"], lambda r: f"{r['h']}x{r['w']}")
        out["sizes_16x512x512"] = next(r for r in res["sizes"] if (r["n"], r["h"], r["w"]) == (16, 512, 512))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("lib")
    ap.add_argument("--part", choices=("cpu", "gpu"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--full", action="store_true", help="every record instead of a count and a sha256 per group (some 300 KB)")
    a = ap.parse_args()
    lib = _native._open(Path(a.lib).resolve())
    if a.part == "cpu":
        if torch.cuda.is_available():
            sys.exit("the cpu part passes made-up pointers: run it on a machine without a device")
        res = cpu_part(lib)
    else:
        res = gpu_part(lib)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(dumps(res if a.full else summary(res)))
    print(f"{a.out}: {len(res.get('refused', res.get('outputs', [])))} records")


if __name__ == "__main__":
    main()
