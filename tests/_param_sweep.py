"""The yardstick of the parameter sweep (tests/test_param_sweep_cpu.py, tests/test_param_sweep_gpu.py): the value sweeps
(tests/_value_sweep.py) walk every pixel VALUE through the per-pixel kernels with their parameters fixed; here the pixels are few and the
PARAMETERS are swept -- the rows a caller of the slide-level API passes that did not come from the tile at hand.  numpy and torch CPU only.

Pixels (per element type, :func:`pixels`): the grey axis and the six channel sweeps of ``_value_sweep._axis_and_sweeps`` over the 256
levels, 4096 seeded colours (floats: 4096 seeded uniform triples of [0, 1)) and the 0.5-grey pad, every member inside [0, 1].  One tile
per parameter row, in two layouts: 64 x 96 (H * W % 16 == 0, the pack path) and 77 x 79 (odd W, odd H * W: the single-element path), the
pixel list permuted per tile with a seed.  At most MAX_ROWS rows per call.

Families (each a :class:`Rows`: names, float32 parameters as the kernels read them, which rows are ESTIMATED -- what an estimate of some
tile or slide gives -- and which CONSTRUCTED, and which lie inside the family's verified domain):

    he_sources()   H&E bases and maxC (sx_macenko_apply, sx_macenko_separate_apply)      domain: HE_COND_CAP, HE_SCALE_RANGE, HE_CONC_GAIN_CAP
    he_factors()   (alpha, beta) of the H and E concentrations                            domain: HE_ALPHA_RANGE, HE_BETA_CAP
    bases()        three-stain bases (sx_deconv_apply / _separate / _combine / _quantify) domain: BASIS_DET_FLOOR
    reinhard()     LAB statistics (sx_reinhard_apply_stats)                               domain: REINHARD_GAIN_RANGE, REINHARD_MEAN_RANGE
    tables()       lookup tables (sx_hm_apply_tables)                                     domain: entries finite, inside 0..255
    luminosity()   luminance percentiles Y_p (sx_luminosity_apply)                        domain: LUMINOSITY_LP_FLOOR, Y_p finite

A row is inside its domain where the project's float32 model stays within a QUARTER of the project's unchanged bound of the float64
reference (tests/test_param_sweep_cpu.py measures it and prints the figures); the constants below are those measurements rounded
inwards.  Domains are narrowed, bounds are not widened.  The float64 references are the project's restatements (vs.macenko64,
vs.separation64, vs.reinhard64, tests/_deconv_numpy.py, tests/_luminosity_numpy.py, sn.lookup), evaluated per row from the float32 row as
it is, once per element type and session.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from oracle import stain_oracle as so
from stainx_amd import stain_basis, synth
from tests import _deconv_numpy as dn
from tests import _hm_slide_numpy as sn
from tests import _luminosity_numpy as ln
from tests import _value_sweep as vs

F32, F64 = np.float32, np.float64
TINY = np.finfo(F32)
DENORMAL = F32(1e-41)
LAYOUTS = {"packs": (64, 96), "odd": (77, 79)}
MAX_ROWS = 64
DTYPES = {"u8": torch.uint8, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PIXEL_SEEDS = {"u8": 3101, "f32": 3102, "bf16": 3103, "f16": 3104}
RANDOM_PIXELS = 4096
N_PIXELS = 7 * 256 + RANDOM_PIXELS      # without the pad, which is pixel N_PIXELS
SYNTH_TILES = 12                         # he_batch(12, 128, 128, seed0=900): the first one is the value sweep's source
TMC_SYNTH = (1.9705, 1.0308)             # the target maxC that goes with synth.HE_REF

# ------------------------------------------------------------------------------------------------ the verified domains
# (tests/test_param_sweep_cpu.py: inside => the float32 model is within a quarter of the bound of float64; DESIGN.md 5e has the figures)
HE_COND_CAP = 25.0                       # cond(HE) = sigma_max / sigma_min of the (3, 2) basis in float64; both column sums positive (the estimate's sign rule)
HE_SCALE_RANGE = (0.05, 2.5)             # target_max_conc / maxC / |column|, either stain, either reference (maxC finite and positive)
HE_CONC_GAIN_CAP = 20.0                  # concentrations (separation): max(scale) / sigma_min(HE), scale = 1 in the own basis
HE_ALPHA_RANGE = (-1.2, 1.2)             # factors: finite, alpha inside, |beta| <= HE_BETA_CAP (the float32 values of these bounds)
HE_BETA_CAP = 3.0
BASIS_DET_FLOOR = 0.05                   # |det| of a basis of unit columns (and of the target basis)
REINHARD_GAIN_RANGE = (0.1, 2.5)         # ref_std / src_std of L, a and b, either fitted reference (src_std finite and positive)
REINHARD_MEAN_RANGE = (-64.0, 320.0)     # the source mean, any of L, a, b on the 0..255 scale
LUMINOSITY_LP_FLOOR = 0.25               # L_p of the row (gain 400); Y_p finite
LUMINOSITY_GAIN_GAP = 1e-3               # |100 / L_p - 1| at least this, or Y_p exactly 1 (copied): nearer to gain 1 the map is the identity to float32
                                         # rounding and EVERY uint8 element lies within the bound of an integer (L_p 99.9 is inside, the neighbours of 1 are not)
TABLE_RANGE = (0.0, 255.0)


@dataclass
class Rows:
    family: str
    names: list
    estimated: np.ndarray      # (R,) bool
    params: dict               # name -> (R, ...) float32
    inside: np.ndarray         # (R,) bool

    def __len__(self) -> int:
        return len(self.names)

    def chunks(self):
        """Row index slices of at most MAX_ROWS rows: one call each."""
        return [slice(s, min(s + MAX_ROWS, len(self))) for s in range(0, len(self), MAX_ROWS)]

    def index(self, name: str) -> int:
        return self.names.index(name)


def _rows(family: str, entries: list, inside_of) -> Rows:
    """``entries``: (name, estimated, {param: value}); ``inside_of(params_of_row) -> bool``."""
    keys = list(entries[0][2])
    params = {k: np.stack([np.asarray(e[2][k], dtype=F32) for e in entries]) for k in keys}
    with np.errstate(all="ignore"):
        inside = np.array([bool(inside_of({k: params[k][i] for k in keys})) for i in range(len(entries))])
    names = [e[0] for e in entries]
    assert len(set(names)) == len(names), family
    return Rows(family, names, np.array([e[1] for e in entries]), params, inside)


# ------------------------------------------------------------------------------------------------ pixels and tiles
@lru_cache(maxsize=None)
def pixels(kind: str) -> torch.Tensor:
    """(N_PIXELS + 1, 3) of the element type: axis and sweeps, the seeded colours, the pad."""
    dtype, rng = DTYPES[kind], np.random.default_rng(PIXEL_SEEDS[kind])
    if dtype == torch.uint8:
        levels = torch.arange(256, dtype=torch.uint8)
        parts = [levels[:, None].expand(-1, 3)]
        for fixed in vs.FIXED:      # (vs.set_a_small: the fixed members as levels)
            for c in range(3):
                px = torch.tensor([round(255 * v) for v in fixed], dtype=torch.uint8).repeat(256, 1)
                px[:, c] = levels
                parts.append(px)
        swept = torch.cat(parts)
        random = torch.from_numpy(rng.integers(0, 256, size=(RANDOM_PIXELS, 3), dtype=np.uint8))
        pad = torch.tensor([[128, 128, 128]], dtype=torch.uint8)
    else:
        swept = vs._axis_and_sweeps((torch.arange(256, dtype=torch.float32) / 255.0).to(dtype))
        random = torch.from_numpy(rng.random((RANDOM_PIXELS, 3), dtype=F32)).to(dtype)
        pad = torch.full((1, 3), 0.5, dtype=dtype)
    out = torch.cat([swept, random, pad])
    assert out.shape == (N_PIXELS + 1, 3) and float(out.float().min()) >= 0.0 and float(out.float().max()) <= (255.0 if dtype == torch.uint8 else 1.0)
    return out


@lru_cache(maxsize=None)
def x32(kind: str) -> np.ndarray:
    """(N_PIXELS + 1, 3) float32 unit values: what every kernel makes of an element."""
    px = pixels(kind)
    return so.to_unit_float(px.numpy()) if px.dtype in (torch.uint8, torch.float32) else px.float().numpy()


@lru_cache(maxsize=None)
def tile_index(layout: str, n: int) -> np.ndarray:
    """(n, H * W) int64: the pixel of the list at every position of tile t -- a permutation seeded by (layout, t), so tile t is the same
    tile in a call of n tiles and in a call of its own."""
    h, w = LAYOUTS[layout]
    assert h * w >= N_PIXELS + 1 and n <= MAX_ROWS
    base = np.full(h * w, N_PIXELS, dtype=np.int64)
    base[:N_PIXELS] = np.arange(N_PIXELS)
    return np.stack([np.random.default_rng([41 if layout == "packs" else 43, t]).permutation(base) for t in range(n)])


def images(kind: str, layout: str, n: int, channels_last: bool = False) -> torch.Tensor:
    h, w = LAYOUTS[layout]
    nhwc = pixels(kind)[torch.from_numpy(tile_index(layout, n))].view(n, h, w, 3)
    return nhwc.contiguous() if channels_last else nhwc.permute(0, 3, 1, 2).contiguous()


def spread(per_row: np.ndarray, layout: str) -> np.ndarray:
    """(R, N_PIXELS + 1, K) per row and pixel -> (R, K, H, W) in the layout's tiles (row t in tile t)."""
    h, w = LAYOUTS[layout]
    r, _, k = per_row.shape
    got = np.take_along_axis(per_row, tile_index(layout, r)[:, :, None], axis=1)
    return np.ascontiguousarray(got.reshape(r, h, w, k).transpose(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ estimates by the oracle
@lru_cache(maxsize=None)
def real_quadrants() -> np.ndarray:
    """(24, 3, 512, 512) uint8: the four quadrants of the six real H&E images."""
    x = ln.real_images()
    return np.ascontiguousarray(np.concatenate([x[:, :, r:r + 512, c:c + 512] for r in (0, 512) for c in (0, 512)]))


@lru_cache(maxsize=None)
def synth_tiles() -> np.ndarray:
    return synth.he_batch(SYNTH_TILES, 128, 128, seed0=900).numpy()


@lru_cache(maxsize=None)
def he_estimates() -> tuple:
    """(names, HE (R, 3, 2), maxC (R, 2)) float32: the oracle's estimates of the synthetic tiles, and of the real quadrants as the golden
    fixture records them (tests/golden/g11_real_tissue.npz: q512_u8_he / _max_c, made by tests/golden/make_golden.py with the oracle)."""
    od = so.optical_density(so.to_unit_float(synth_tiles()))
    est = [so.macenko_tile_params(od[i], signs="positive_sum") for i in range(SYNTH_TILES)]
    with np.load(vs.GOLDEN / "g11_real_tissue.npz", allow_pickle=False) as g:
        he_real, mc_real = g["q512_u8_he"].astype(F32), g["q512_u8_max_c"].astype(F32)
    names = [f"synth seed {900 + i}" for i in range(SYNTH_TILES)] + [f"real quadrant {i}" for i in range(len(he_real))]
    he = np.concatenate([np.stack([p["he"] for p in est]).astype(F32), he_real])
    max_c = np.concatenate([np.stack([p["max_c"] for p in est]).astype(F32), mc_real])
    assert np.isfinite(he).all() and np.isfinite(max_c).all() and (max_c > 0).all()
    return names, he, max_c


def he_references() -> dict:
    """The two fitted references (stain_matrix, target_max_conc): the real-tissue one and synth.HE_REF with its TMC."""
    st = vs.statistics()
    return {"real": (st["sm"], st["tmc"]), "synth": (np.asarray(synth.HE_REF, dtype=F32), np.asarray(TMC_SYNTH, dtype=F32))}


def moved(he: np.ndarray, t: float) -> np.ndarray:
    """E moved towards H (t < 1) or away from it (t > 1) along the chord, both columns unit length: t = 1 is the basis itself."""
    he = he.astype(F64)
    h, e = he[:, 0] / np.linalg.norm(he[:, 0]), he[:, 1] / np.linalg.norm(he[:, 1])
    e2 = h + t * (e - h)
    return np.stack([h, e2 / np.linalg.norm(e2)], axis=1).astype(F32)


def he_cond(he: np.ndarray) -> float:
    s = np.linalg.svd(np.asarray(he, dtype=F64).reshape(3, 2), compute_uv=False)
    return float(s[0] / s[1]) if s[1] > 0 else float("inf")


def he_angle(he: np.ndarray) -> float:
    he = np.asarray(he, dtype=F64).reshape(3, 2)
    c = he[:, 0] @ he[:, 1] / (np.linalg.norm(he[:, 0]) * np.linalg.norm(he[:, 1]))
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def he_scales(he: np.ndarray, max_c: np.ndarray, tmc) -> np.ndarray:
    """(2,) the factor between a unit optical density along a stain vector and its normalised concentration: target_max_conc / maxC
    over the column's length (a column of half the length doubles the concentration)."""
    with np.errstate(all="ignore"):
        return np.asarray(tmc, dtype=F64) / np.asarray(max_c, dtype=F64) / np.linalg.norm(np.asarray(he, dtype=F64).reshape(3, 2), axis=0)


def he_conc_gain(he: np.ndarray, scale=None) -> float:
    """The gain of the concentration map C = diag(scale) pinv(HE) OD: max(scale) / sigma_min(HE) (own basis: scale 1)."""
    s = np.linalg.svd(np.asarray(he, dtype=F64).reshape(3, 2), compute_uv=False)
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(1.0 if scale is None else scale)) / s[1]) if s[1] > 0 else float("inf")


def _he_inside(p: dict) -> bool:
    he, max_c = p["he"].astype(F64), p["max_c"].astype(F64)
    if not (np.isfinite(he).all() and np.isfinite(max_c).all() and (max_c > 0).all() and (he.sum(axis=0) > 0).all() and he_cond(he) <= HE_COND_CAP):
        return False
    scales = np.stack([he_scales(he, max_c, tmc) for _, tmc in he_references().values()])
    return bool((scales >= HE_SCALE_RANGE[0]).all() and (scales <= HE_SCALE_RANGE[1]).all())


HE_MOVES = (1.0, 0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 2.0, 4.0)


@lru_cache(maxsize=None)
def he_sources() -> Rows:
    names, he, max_c = he_estimates()
    base_he, base_mc = he[0], max_c[0]      # (vs.statistics()'s source)
    entries = [(n, True, {"he": he[i], "max_c": max_c[i]}) for i, n in enumerate(names)]
    for t in HE_MOVES:
        entries.append((f"E moved t={t:g}", False, {"he": moved(base_he, t), "max_c": base_mc}))
    for col, norm in ((0, 0.5), (1, 0.5), (0, 2.0), (1, 2.0)):
        scaled = base_he.copy()
        scaled[:, col] *= F32(norm)
        entries.append((f"column {col} norm {norm:g}", False, {"he": scaled, "max_c": base_mc}))
    flipped = base_he.copy()
    flipped[:, 1] = -flipped[:, 1]
    rank1 = base_he.copy()
    rank1[:, 1] = 0
    entries += [("E sign flipped", False, {"he": flipped, "max_c": base_mc}), ("rank-1 HE", False, {"he": rank1, "max_c": base_mc}),
                ("zero HE", False, {"he": np.zeros((3, 2), F32), "max_c": base_mc})]
    for what, value in (("maxC / 4", base_mc / 4), ("maxC x 1", base_mc), ("maxC x 4", base_mc * 4), ("maxC 1e-30", [1e-30, base_mc[1]]), ("maxC 1e30", [base_mc[0], 1e30]),
                        ("maxC denormal", [DENORMAL, base_mc[1]]), ("maxC 0", [0.0, base_mc[1]]), ("maxC negative", [-base_mc[0], base_mc[1]]),
                        ("maxC Inf", [base_mc[0], np.inf]), ("maxC NaN", [np.nan, base_mc[1]])):
        entries.append((what, False, {"he": base_he, "max_c": value}))
    return _rows("he_sources", entries, _he_inside)


def _factor_inside(p: dict) -> bool:
    a, b = p["alpha"], p["beta"]
    return np.isfinite(a).all() and np.isfinite(b).all() and (a >= F32(HE_ALPHA_RANGE[0])).all() and (a <= F32(HE_ALPHA_RANGE[1])).all() and (np.abs(b) <= F32(HE_BETA_CAP)).all()


@lru_cache(maxsize=None)
def he_factors() -> Rows:
    """(alpha, beta) rows, applied with the value sweep's source.  Estimated: what MacenkoAugment.sample_factors draws with its
    defaults (alpha in [0.8, 1.2], beta in [-0.2, 0.2]) -- the identity, its four extreme corners, seeded draws."""
    rng = np.random.default_rng(3110)
    entries = [("identity", True, {"alpha": [1, 1], "beta": [0, 0]})]
    for a0, a1, b0, b1 in ((0.8, 0.8, -0.2, -0.2), (1.2, 1.2, 0.2, 0.2), (0.8, 1.2, 0.2, -0.2), (1.2, 0.8, -0.2, 0.2)):
        entries.append((f"corner {a0:g} {a1:g} {b0:g} {b1:g}", True, {"alpha": [a0, a1], "beta": [b0, b1]}))
    for i in range(4):
        entries.append((f"draw {i}", True, {"alpha": 0.8 + 0.4 * rng.random(2), "beta": -0.2 + 0.4 * rng.random(2)}))
    entries += [("alpha H = 0", False, {"alpha": [0, 1], "beta": [0, 0]}), ("alpha E = 0", False, {"alpha": [1, 0], "beta": [0, 0]}),
                ("alpha negative", False, {"alpha": [-1, 1], "beta": [0, 0]}), ("alpha 0.5", False, {"alpha": [0.5, 0.5], "beta": [0, 0]}),
                ("beta 0.1", False, {"alpha": [1, 1], "beta": [0.1, -0.1]}), ("alpha 1.1 beta -0.05", False, {"alpha": [1.1, 0.9], "beta": [-0.05, 0.05]}),
                ("beta +3", False, {"alpha": [1, 1], "beta": [3, 3]}), ("beta -3", False, {"alpha": [1, 1], "beta": [-3, -3]}),
                ("alpha 4", False, {"alpha": [4, 4], "beta": [0, 0]}), ("alpha NaN", False, {"alpha": [np.nan, 1], "beta": [0, 0]}),
                ("beta NaN", False, {"alpha": [1, 1], "beta": [0, np.nan]}), ("alpha Inf", False, {"alpha": [np.inf, 1], "beta": [0, 0]}),
                ("beta -Inf", False, {"alpha": [1, 1], "beta": [-np.inf, 0]})]
    return _rows("he_factors", entries, _factor_inside)


# ---- three-stain bases
def _unit_columns(b: np.ndarray) -> np.ndarray:
    return b / np.linalg.norm(b, axis=0, keepdims=True)


def basis_with_det(det: float, seed: int) -> np.ndarray:
    """A seeded (3, 3) float32 basis of unit columns with |det| = ``det`` (to float32 rounding): the third column of a random basis is
    turned towards the plane of the first two until the determinant is the one asked for."""
    rng = np.random.default_rng(seed)
    b = _unit_columns(np.abs(rng.normal(size=(3, 3))) + 0.1)
    n = np.cross(b[:, 0], b[:, 1])
    in_plane = _unit_columns((b[:, 0] + b[:, 1])[:, None])[:, 0]
    sin = det / np.linalg.norm(n)      # det = |a x b| sin(angle between c and the plane)
    assert 0 < sin < 1
    c = np.sqrt(1 - sin * sin) * in_plane + sin * n / np.linalg.norm(n)
    out = np.stack([b[:, 0], b[:, 1], c], axis=1)
    assert abs(abs(np.linalg.det(out)) - det) <= 1e-9
    return out.astype(F32)


def _basis_inside(p: dict) -> bool:
    ok = True
    for key in ("basis", "target"):
        b = p[key].astype(F64)
        ok = ok and np.isfinite(b).all() and abs(np.linalg.det(b)) >= BASIS_DET_FLOOR and np.allclose(np.linalg.norm(b, axis=0), 1.0, atol=1e-3)
    return ok


BASIS_DETS = (0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 1e-3, 1e-6)


@lru_cache(maxsize=None)
def bases() -> Rows:
    """``target``: the basis the tile is rebuilt with by apply(target=...): never the row's own (that map is the identity, whose uint8
    reference is all integers) -- another named basis, ``hed`` for the constructed rows but for those that say otherwise."""
    named = {n: stain_basis(n).numpy().astype(F32) for n in ("hed", "hdab", "he")}
    entries = [(n, True, {"basis": named[n], "target": named[{"hed": "hdab", "hdab": "he", "he": "hed"}[n]]}) for n in named]
    names, he, _ = he_estimates()
    for n, h in zip(names, he):
        comp = dn.complement(h).astype(F32)
        entries.append((f"complement {n}", True, {"basis": comp, "target": named["he"]}))
    for i, det in enumerate(BASIS_DETS):
        entries.append((f"det {det:g}", False, {"basis": basis_with_det(det, 3120 + i), "target": named["hed"]}))
    hed = named["hed"]
    entries += [("hed columns 1 2 0", False, {"basis": hed[:, [1, 2, 0]], "target": hed}), ("hed columns 2 1 0", False, {"basis": hed[:, [2, 1, 0]], "target": named["hdab"]}),
                ("hed to permuted hed", False, {"basis": hed, "target": hed[:, [1, 0, 2]]}), ("hdab to det 0.2", False, {"basis": named["hdab"], "target": basis_with_det(0.2, 3121)}),
                ("det 0.5 to hed", False, {"basis": basis_with_det(0.5, 3120), "target": hed})]
    singular = hed.copy()
    singular[:, 2] = singular[:, 0]
    nan = hed.copy()
    nan[1, 1] = np.nan
    entries += [("singular: two equal columns", False, {"basis": singular, "target": hed}), ("singular: zero column", False, {"basis": hed * np.array([1, 0, 1], F32), "target": hed}),
                ("NaN basis", False, {"basis": nan, "target": hed}), ("NaN target", False, {"basis": hed, "target": nan})]
    return _rows("bases", entries, _basis_inside)


def basis_defined(rows: Rows) -> np.ndarray:
    """(R,) bool: rows whose pixel values are defined at all -- finite and not exactly singular (the header: a singular basis on the
    device is undefined; a NaN row is copied by the masked call only)."""
    with np.errstate(all="ignore"):
        return np.array([bool(np.isfinite(rows.params["basis"][i]).all() and np.isfinite(rows.params["target"][i]).all()
                              and np.linalg.matrix_rank(rows.params["basis"][i].astype(F64)) == 3) for i in range(len(rows))])


# ---- Reinhard statistics
def reinhard_references() -> dict:
    """Two fitted references -- reference_tile(128, 128), the value sweep's, and a darker synthetic tile -- and one with ref_std = 0 (every
    pixel becomes the reference's mean colour).  Both keep ref_std / src_std of every estimated row inside REINHARD_GAIN_RANGE.  A real-tissue
    fit (a quadrant's, or c224_reinhard_ref_* of the golden set) against the synthetic sources has a ratio of 5, where the float32 oracle
    was 2.8e-5 ... 6.5e-5 from float64 when the references were chosen: outside the domain; the rows std x 0.5, std x 0.1
    stand for such pairs."""
    st = vs.statistics()
    dark = so.reinhard_fit(synth.he_tile(128, 128, 43, 1.3).numpy())
    return {"synth": (st["ref_mean"], st["ref_std"]), "synth dark": (dark[0].astype(F32), dark[1].astype(F32)), "ref_std 0": (st["ref_mean"], np.zeros(3, F32))}


def _reinhard_inside(p: dict) -> bool:
    mean, std = p["mean"].astype(F64), p["std"].astype(F64)
    if not (np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()):
        return False
    gains = np.stack([np.asarray(rs, dtype=F64) / std for name, (_, rs) in reinhard_references().items() if name != "ref_std 0"])
    return gains.min() >= REINHARD_GAIN_RANGE[0] and gains.max() <= REINHARD_GAIN_RANGE[1] and (mean >= REINHARD_MEAN_RANGE[0]).all() and (mean <= REINHARD_MEAN_RANGE[1]).all()


@lru_cache(maxsize=None)
def reinhard() -> Rows:
    entries = []
    for i, tile in enumerate(synth_tiles()):
        mean, std = so.reinhard_fit(tile[None])
        entries.append((f"synth seed {900 + i}", True, {"mean": mean, "std": std}))
    for i, quad in enumerate(real_quadrants()):
        mean, std = so.reinhard_fit(quad[None])
        entries.append((f"real quadrant {i}", True, {"mean": mean, "std": std}))
    st = vs.statistics()
    mean, std = st["mean"], st["std"]
    entries.append(("pooled synth", True, {"mean": mean, "std": std}))
    for f in (0.5, 0.8, 1.25, 2.0, 1e-1, 1e-2, 1e-3, 1e4):
        entries.append((f"std x {f:g}", False, {"mean": mean, "std": std * F32(f)}))
    for what, value in (("std 0", [0.0, std[1], std[2]]), ("std denormal", [std[0], DENORMAL, std[2]]), ("std negative", [std[0], std[1], -std[2]]), ("std Inf", [np.inf, std[1], std[2]]),
                        ("std NaN", [std[0], np.nan, std[2]]), ("mean NaN", None)):
        entries.append((what, False, {"mean": mean, "std": value} if value is not None else {"mean": [mean[0], np.nan, mean[2]], "std": std}))
    for shift in (50.0, -50.0, 10.0, -10.0):
        entries.append((f"mean {shift:+g}", False, {"mean": mean + F32(shift), "std": std}))
    return _rows("reinhard", entries, _reinhard_inside)


# ---- lookup tables
def _table_inside(p: dict) -> bool:
    t = p["lut"]
    return np.isfinite(t).all() and (t >= TABLE_RANGE[0]).all() and (t <= TABLE_RANGE[1]).all()


@lru_cache(maxsize=None)
def tables() -> Rows:
    k = np.arange(256, dtype=F32)
    identity = np.broadcast_to(k, (3, 256)).copy()
    entries = [("identity", True, {"lut": identity})]
    for seed in (5, 6, 7, 8):
        entries.append((f"monotone seed {seed}", True, {"lut": vs.monotone_tables(seed)[0]}))
    ref_hists = so.hm_fit(synth.reference_tile(128, 128).numpy())
    sources = np.concatenate([synth_tiles()[:3], real_quadrants()[:3, :, :128, :128]])
    counts = sn.bincounts(sources)
    luts = sn.tables(counts, np.full(len(sources), 128 * 128), ref_hists)
    for i in range(len(sources)):
        entries.append((f"tables of counts {i}", True, {"lut": luts[i]}))

    def with_entries(values, base=identity):
        """The identity with ``values`` written over its entries in turn, each channel starting at another one."""
        values = np.asarray(values, dtype=F32)
        out = base.copy()
        for c in range(3):
            out[c] = np.roll(np.resize(values, 256), 85 * c)
        return out

    top = F32(255.0)
    entries += [("reversed", False, {"lut": identity[:, ::-1].copy()}), ("constant 0", False, {"lut": np.zeros((3, 256), F32)}), ("constant 255", False, {"lut": np.full((3, 256), 255, F32)}),
                ("constant 127.5", False, {"lut": np.full((3, 256), 127.5, F32)}), ("k + 0.5", False, {"lut": np.minimum(identity + F32(0.5), top)}),
                ("k + 0.999", False, {"lut": np.minimum(identity + F32(0.999), top)}), ("255 and the float below", False, {"lut": with_entries([255.0, np.nextafter(top, F32(0))])}),
                ("-0.0", False, {"lut": with_entries([-0.0, 0.0, 3.0])}), ("denormal", False, {"lut": with_entries([DENORMAL, TINY.smallest_subnormal, 7.0])}),
                ("the float above 255", False, {"lut": with_entries([np.nextafter(top, F32(300)), 12.0])}), ("255.5", False, {"lut": with_entries([255.5, 100.0])}),
                ("256", False, {"lut": with_entries([256.0, 20.0])}), ("300", False, {"lut": with_entries([300.0, 511.0, 512.0, 30.0])}), ("1e9", False, {"lut": with_entries([1e9, 3e38, 40.0])}),
                ("k + 0.5 up to 255.5", False, {"lut": identity + F32(0.5)}), ("-0.5", False, {"lut": with_entries([-0.5, 50.0])}), ("-1", False, {"lut": with_entries([-1.0, -255.0, -256.0, -1e9, 60.0])}),
                ("NaN", False, {"lut": with_entries([np.nan, 70.0])}), ("+Inf", False, {"lut": with_entries([np.inf, 80.0])}), ("-Inf", False, {"lut": with_entries([-np.inf, 90.0])}),
                ("all NaN", False, {"lut": np.full((3, 256), np.nan, F32)})]
    return _rows("tables", entries, _table_inside)


# ---- luminosity rows
def y_of_lightness(l_p: float) -> np.float32:
    """The float32 luminance whose L* is ``l_p`` (the inverse of ln.lightness)."""
    f = (l_p + 16.0) / 116.0
    return F32(f ** 3 if f ** 3 > 0.008856 else (f - 16.0 / 116.0) / 7.787)


def _luminosity_inside(p: dict) -> bool:
    y = float(p["y"])
    l_p = float(ln.lightness(y))
    return bool(np.isfinite(y) and l_p >= LUMINOSITY_LP_FLOOR and (y == 1.0 or abs(100.0 / l_p - 1.0) >= LUMINOSITY_GAIN_GAP))


LUMINOSITY_LP = (99.9, 99.0, 90.0, 75.0, 50.0, 30.0, 10.0, 3.0, 1.0, 0.3, 0.1)
ESTIMATED_LP = 10.0      # rows with L_p at least this are what the 95th percentile of a stained tile gives; darker rows are constructed


@lru_cache(maxsize=None)
def luminosity() -> Rows:
    one = F32(1.0)
    entries = [(f"L_p {l_p:g}", l_p >= ESTIMATED_LP, {"y": y_of_lightness(l_p)}) for l_p in LUMINOSITY_LP]
    y_001 = F32(ln.luminance(np.array([[[[0]], [[0]], [[1]]]], dtype=np.uint8))[0, 0, 0])
    entries += [("Y of uint8 (0, 0, 1)", False, {"y": y_001}), ("L_p 1e-3", False, {"y": y_of_lightness(1e-3)}), ("L_p 1e-6", False, {"y": y_of_lightness(1e-6)}),
                ("the float below 1", False, {"y": np.nextafter(one, F32(0))}), ("1", True, {"y": one}), ("the float above 1", False, {"y": np.nextafter(one, F32(2))}),
                ("1.5", False, {"y": 1.5}), ("10", False, {"y": 10.0}), ("FLT_MAX", False, {"y": TINY.max}), ("Inf", False, {"y": np.inf}),
                ("smallest normal", False, {"y": TINY.tiny}), ("denormal", False, {"y": DENORMAL}), ("0", False, {"y": 0.0}), ("-0.0", False, {"y": -0.0}),
                ("negative", False, {"y": -0.25}), ("NaN", False, {"y": np.nan})]
    return _rows("luminosity", entries, _luminosity_inside)


def luminosity_copied(rows: Rows) -> np.ndarray:
    """(R,) bool: rows the header says are copied bit for bit: NaN, L_p <= 0 (in fp64: every Y_p below 1.8e-18) or exactly 1."""
    return ln.gain(rows.params["y"])[1]


# ------------------------------------------------------------------------------------------------ float64 references, per row
def _per_row(fn, n_rows: int) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.stack([fn(i) for i in range(n_rows)])


@lru_cache(maxsize=None)
def he_sources64(kind: str, reference: str) -> np.ndarray:
    """(R, P, 3) float64 un-clamped levels: vs.macenko64 of every pixel with row r's (HE, maxC) and the reference."""
    rows, x, (sm, tmc) = he_sources(), x32(kind), he_references()[reference]
    return _per_row(lambda i: vs.macenko64(x, rows.params["he"][i], rows.params["max_c"][i], sm, tmc)["raw"], len(rows))


@lru_cache(maxsize=None)
def he_separation64(kind: str, reference: str) -> dict:
    """vs.separation64 per row: ``conc`` (R, P, 2) own-basis concentrations, ``scale`` (R, 2) = tmc / maxC, ``own`` / ``normalised``
    (R, 2, P, 3) un-clamped H and E levels."""
    rows, x, (sm, tmc) = he_sources(), x32(kind), he_references()[reference]
    parts = []
    with np.errstate(all="ignore"):
        for i in range(len(rows)):
            parts.append(vs.separation64(x, rows.params["he"][i], rows.params["max_c"][i], sm, tmc))
        scale = np.asarray(tmc, dtype=F64)[None] / rows.params["max_c"].astype(F64)
    return {"conc": np.stack([p["conc"] for p in parts]), "scale": scale, "own": np.stack([p["own"].transpose(1, 0, 2) for p in parts]),
            "normalised": np.stack([p["normalised"].transpose(1, 0, 2) for p in parts])}


@lru_cache(maxsize=None)
def he_factors64(kind: str, own_basis: bool) -> np.ndarray:
    rows, x, st = he_factors(), x32(kind), vs.statistics()
    return _per_row(lambda i: vs.macenko64(x, st["he"], st["max_c"], st["sm"], st["tmc"], alpha=rows.params["alpha"][i], beta=rows.params["beta"][i], own_basis=own_basis)["raw"], len(rows))


@lru_cache(maxsize=None)
def combine_input(kind: str) -> np.ndarray:
    """(1, 3, 1, P) float32 concentrations for ``combine``: the pixel list separated with a seeded basis that is no row's (with a row's own
    basis combine(separate(x)) is the identity, all integers on uint8)."""
    with np.errstate(all="ignore"):
        return dn.concentrations(vs._as_tile(x32(kind)), basis_with_det(0.4, 3199)).astype(F32)


@lru_cache(maxsize=None)
def bases64(kind: str) -> dict:
    """tests/_deconv_numpy.py per row, float64: ``conc`` (R, P, 3); un-clamped levels of ``apply`` with dn.ALPHA / dn.BETA, of
    ``target`` (rebuilt with the row's target basis), ``stains`` (R, 3 images, P, 3) and ``combine`` of :func:`combine_input`.
    Rows that are not :func:`basis_defined` hold NaN."""
    rows, tile = bases(), vs._as_tile(x32(kind))
    ok = basis_defined(rows)
    out = {"conc": [], "apply": [], "target": [], "stains": [], "combine": []}
    nan = np.full((N_PIXELS + 1, 3), np.nan)
    with np.errstate(all="ignore"):
        for i in range(len(rows)):
            if not ok[i]:
                for key in out:
                    out[key].append(np.stack([nan] * 3) if key == "stains" else nan)
                continue
            b, t = rows.params["basis"][i], rows.params["target"][i]
            conc = dn.concentrations(tile, b)
            out["conc"].append(vs._as_pixels(conc))
            out["apply"].append(vs._as_pixels(dn.apply(tile, b, alpha=[dn.ALPHA], beta=[dn.BETA], dtype=F64)))
            out["target"].append(vs._as_pixels(dn.apply(tile, b, target=t, dtype=F64)))
            out["stains"].append(np.stack([vs._as_pixels(img) for img in dn.stain_images(tile, b, dtype=F64)]))
            out["combine"].append(vs._as_pixels(dn.combine(combine_input(kind), b, dtype=F64)))
    return {k: np.stack(v) for k, v in out.items()}


@lru_cache(maxsize=None)
def reinhard64(kind: str, reference: str) -> np.ndarray:
    """(R, P, 3) float64 un-clamped unit values: vs.reinhard64 per row."""
    rows, x, (rm, rs) = reinhard(), x32(kind), reinhard_references()[reference]
    return _per_row(lambda i: vs.reinhard64(x, rows.params["mean"][i], rows.params["std"][i], rm, rs)["raw"], len(rows))


@lru_cache(maxsize=None)
def luminosity64(kind: str) -> np.ndarray:
    """(R, P, 3) float64 unit values BEFORE the clamp: tests/_luminosity_numpy.py's map per row (vs.luminosity64's arithmetic); a row that
    is copied through holds the input's unit values."""
    rows, x = luminosity(), x32(kind)
    tile = vs._as_tile(x)
    with np.errstate(all="ignore"):
        f = ln.f_values(tile)
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        g, through = ln.gain(rows.params["y"])
        out = []
        for i in range(len(rows)):
            if through[i]:
                out.append(x.astype(F64))
                continue
            fy2 = np.minimum(g[i] * fy + (16.0 / 116.0) * (1.0 - g[i]), 1.0)
            lin = np.einsum("ij,njhw->nihw", ln.XYZ2RGB, ln.f_inv(np.stack([fy2 + (fx - fy), fy2, fy2 - (fy - fz)], axis=1)) * ln.WHITE)
            curve = lin > 0.0031308
            out.append(vs._as_pixels(np.where(curve, 1.055 * vs._pow(curve, lin, 1.0 / 2.4) - 0.055, 12.92 * lin)))
    return np.stack(out)


def tables_expected(kind: str, layout: str, rows: slice, channels_last: bool = False) -> torch.Tensor:
    """sn.lookup of the layout's tiles with the tables of ``rows`` (exact arithmetic: the expected BITS), typed as the input."""
    luts = tables().params["lut"][rows]
    src = images(kind, layout, len(luts), channels_last)
    x = src.numpy() if src.dtype in (torch.uint8, torch.float32) else src.float().numpy()
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.ascontiguousarray(sn.lookup(x, luts, -1 if channels_last else 1))).to(src.dtype)
