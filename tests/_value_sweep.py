"""The yardstick of the value-domain sweeps (tests/test_value_sweep_cpu.py, tests/test_value_sweep_gpu.py): input sets that walk the per-pixel
kernels through EVERY value an element type can hold, and a plain float64 restatement of the pixel arithmetic to hold them to.  numpy only.

A set is a list of pixels (P, 3) in its element type plus layouts: NCHW tiles that hold every pixel of the list once, in a seeded
permutation (so that a value does not always meet the same lane of a pack), filled up with 0.5 grey; one layout with H * W % 16 == 0 (the
pack path of every kernel) and one with odd W and odd H * W (the single-element path).  Every reference is evaluated ONCE per pixel of the
list, in float64, in slices of 2^20 pixels, and carried to a layout through its index -- both layouts and every test of a session share it.

    A  all 2^24 uint8 colours, one 4096 x 4096 tile (uint8);
    B  every 16-bit pattern of bfloat16 / float16, non-finite ones included, as the grey axis (v, v, v) and as each channel swept with the
       other two fixed at (0.85, 0.55, 0.75) and at (0.3, 0.2, 0.5);
    C  float32: the k / 255 lattice with its +-1 and +-2 ulp neighbours, the 33 values either side of every branch point of the input
       side, denormals, -0.0, values a little outside [0, 1], 2^20 uniform values in [0, 1) and 2^18 in [-1, 2] -- as grey axis, channel
       sweeps and random triples; +-Inf, NaN and +-FLT_MAX as a group of their own (pixels with a member of it are out of every domain);
       and two tiles that hold lattice values only, so that tiles that pass the 8-bit code gates sit beside tiles that do not.

    A_small  uint8 through the single-element path of the stain sweeps: every level in every channel and 2^16 seeded colours, odd layout only
             (set A then runs its 2^24 colours once, in the pack layout: :func:`stain_layouts`);
    K  float32 CONCENTRATIONS for ``ColorDeconvolution.combine`` (:func:`concentration_set`).

    gate_tiles()  float32 tiles for the 8-bit code gates, which mark WHOLE tiles: grey levels, every element one ulp off, one element off.

The stain sweeps (tests/test_value_sweep_stains_gpu.py) add references from the project's restatements, float64 throughout: ``separation``
(two-stain concentrations and H / E levels, own basis and normalised), ``jitter`` (macenko64 with C' = alpha C + beta, the fixed pairs
JITTER dealt to the tiles in turn), ``deconv(name)`` (tests/_deconv_numpy.py: concentrations, apply with factors, apply with the other
basis as target, three stain images), ``luminosity`` (tests/_luminosity_numpy.py's map for the rows LUMINOSITY_Y, with the way every
branch went) and :func:`combine64`; ``luminosity_domain`` is every member in [0, 1].

Masks per pixel: ``finite``; ``reinhard_domain`` (every member in [-1, 2]) and ``macenko_domain`` (every member in [-1/512, 2]: the optical
density -log((255 x + 1) / 240) has its pole at -1/255), the domains on which the kernels are held to the float64 reference.

The source statistics are FIXED (the error gain of both transforms depends on them): see :func:`statistics`.
"""
from __future__ import annotations

from functools import cached_property, lru_cache
from pathlib import Path

import numpy as np
import torch

from oracle import stain_oracle as so
from stainx_amd import stain_basis, synth
from tests import _deconv_numpy as dn
from tests import _luminosity_numpy as ln
from tests import _quantify_numpy as qn

F32 = np.float32
SLICE = 1 << 20
GOLDEN = Path(__file__).resolve().parent / "golden"
FIXED = ((0.85, 0.55, 0.75), (0.3, 0.2, 0.5))      # the other two channels of a one-channel sweep
THRESHOLDS = (0.5, 0.8, 0.9)                       # luminosity thresholds of the rule tests
REINHARD_TOL = 1e-4                                # the project's parity bound on [0, 1] (tests/test_siblings_gpu.py, test_per_tile_gpu.py)
TRIPLE_DOMAIN = (-0.25, 1.25)                      # the Reinhard domain of set C's random triples (Sweep.reinhard_domain says why)
MIN_BRANCH_PIXELS = 1000                           # coverage: in-domain pixels on either side of every branch, per float set
CONC_TOL = qn.CONC_TOL                             # the project's bound on a float32 concentration against float64
LUMINOSITY_TOL = 1e-4                              # the project's bound of the luminosity apply pass on [0, 1] (tests/test_luminosity_gpu.py)
DECONV_NAMES = ("hed", "hdab")
OTHER_BASIS = {"hed": "hdab", "hdab": "hed"}       # ColorDeconvolution(name, target=the other basis)
# (alpha, beta) of the (H, E) concentrations, one pair per tile in turn: the identity, a mild pair, and a corner of what
# MacenkoAugment.sample_factors draws with its defaults sigma1 = sigma2 = 0.2 (alpha in [0.8, 1.2], beta in [-0.2, 0.2])
JITTER = (((1.0, 1.0), (0.0, 0.0)), ((1.1, 0.92), (0.03, -0.02)), ((1.2, 0.8), (0.2, -0.2)))
# the luminance percentiles Y_p of the luminosity rows, as the float32 the kernel reads: L_p = 30, 75 and 100 (gains 3.33, 1.33 and 1)
LUMINOSITY_Y = tuple(float(F32(((l_p + 16.0) / 116.0) ** 3)) for l_p in (30.0, 75.0, 100.0))
QUANTIFY_BINNING = (5, 64)                         # bin_log2, zero_bin
POLE_BAND = 1e-4                                   # quantify: a member whose float64 255 x + 1 lies within this of zero is not decided
COMBINE_DOMAIN = 12.0                              # the concentration set: every member finite with |C| <= 12

# ------------------------------------------------------------------------------------------------ the float64 reference
_RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])      # oracle/stain_oracle.py:232
_XYZ2RGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])
_D65 = np.array([0.95047, 1.0, 1.08883])


def _pow(cond: np.ndarray, base: np.ndarray, exponent: float) -> np.ndarray:
    """base ** exponent where ``cond`` (the branch that is taken), 1 elsewhere: no warning from the branch that is not."""
    return np.power(np.where(cond, base, 1.0), exponent)


def rgb_to_lab64(x: np.ndarray) -> dict:
    """so.rgb_to_lab on (P, 3) unit pixels in float64, same constants, branches and order: ``lab`` (L * 2.55, a + 128, b + 128), and which
    branch every member took: ``gamma_in`` (x > 0.04045) and ``f`` (X/Xn, Y, Z/Zn > 0.008856)."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(x, dtype=np.float64)      # (the cast of a signalling NaN raises "invalid" too)
        gamma = x > 0.04045
        lin = np.where(gamma, _pow(gamma, (x + 0.055) / 1.055, 2.4), x / 12.92)
        xyz = np.stack([lin[:, 0] * m[0] + lin[:, 1] * m[1] + lin[:, 2] * m[2] for m in _RGB2XYZ], axis=1) / _D65
        cube = xyz > 0.008856
        f = np.where(cube, _pow(cube, xyz, 1.0 / 3.0), 7.787 * xyz + 16.0 / 116.0)
        lab = np.stack([(116.0 * f[:, 1] - 16.0) * 2.55, 500.0 * (f[:, 0] - f[:, 1]) + 128.0, 200.0 * (f[:, 1] - f[:, 2]) + 128.0], axis=1)
    return {"lab": lab, "gamma_in": gamma, "f": cube}


def lab_to_rgb64(lab: np.ndarray) -> dict:
    """so.lab_to_rgb on (P, 3) in float64: ``rgb`` clamped to [0, 1], ``f_inv`` (fx, fy, fz > 0.2068966), ``gamma_out`` (linear > 0.0031308)."""
    with np.errstate(invalid="ignore", over="ignore"):
        fy = (lab[:, 0] / 2.55 + 16.0) / 116.0
        fx = (lab[:, 1] - 128.0) / 500.0 + fy
        fz = fy - (lab[:, 2] - 128.0) / 200.0
        t = np.stack([fx, fy, fz], axis=1)
        cube = t > 0.2068966
        xyz = np.where(cube, t ** 3, (t - 16.0 / 116.0) / 7.787) * _D65
        lin = np.stack([xyz[:, 0] * m[0] + xyz[:, 1] * m[1] + xyz[:, 2] * m[2] for m in _XYZ2RGB], axis=1)
        gamma = lin > 0.0031308
        rgb = np.where(gamma, 1.055 * _pow(gamma, lin, 1.0 / 2.4) - 0.055, 12.92 * lin)
    return {"rgb": np.clip(rgb, 0.0, 1.0), "raw": rgb, "f_inv": cube, "gamma_out": gamma}


def reinhard64(x: np.ndarray, mean, std, ref_mean, ref_std) -> dict:
    """The Reinhard apply with GIVEN statistics (oracle/stain_oracle.py:289-290) in float64; the float32 statistics enter as they are."""
    fwd = rgb_to_lab64(x)
    mean, std, ref_mean, ref_std = (np.asarray(v, dtype=np.float64).reshape(1, 3) for v in (mean, std, ref_mean, ref_std))
    with np.errstate(invalid="ignore", over="ignore"):
        back = lab_to_rgb64((fwd["lab"] - mean) / (std + 1e-8) * ref_std + ref_mean)
    return {"out": back["rgb"], "raw": back["raw"], "lab": fwd["lab"], "gamma_in": fwd["gamma_in"], "f": fwd["f"], "f_inv": back["f_inv"], "gamma_out": back["gamma_out"]}


def optical_density64(x: np.ndarray) -> np.ndarray:
    """OD = -log((255 x + 1) / 240) of (P, 3) unit pixels in float64 (oracle/stain_oracle.py:58)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return -np.log((np.asarray(x, dtype=np.float64) * 255.0 + 1.0) / 240.0)


def concentrations64(x: np.ndarray, he) -> np.ndarray:
    """(P, 2) float64: the least-squares concentrations of (P, 3) unit pixels in the basis ``he`` (oracle/stain_oracle.py:117)."""
    he = np.asarray(he, dtype=np.float64).reshape(3, 2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.linalg.lstsq(he, optical_density64(x).T, rcond=None)[0].T


def rebuild64(conc: np.ndarray, basis) -> np.ndarray:
    """(P, S) concentrations -> (P, 3) un-clamped levels 240 exp(-basis C) with a (3, S) basis (oracle/stain_oracle.py:162-164)."""
    basis = np.asarray(basis, dtype=np.float64).reshape(3, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return 240.0 * np.exp(-(conc @ basis.T))


def macenko64(x: np.ndarray, he, max_c, sm, tmc, alpha=None, beta=None, own_basis: bool = False) -> dict:
    """The tail of the Macenko transform with a GIVEN (HE, maxC, SM, targetMaxC) (oracle/stain_oracle.py:58, 117, 162-164) in float64:
    OD = -log((255 x + 1) / 240), least squares, rescale, 240 exp(-OD'), clipped to 0..255.  (P, 3) in; ``out`` (P, 3), ``raw`` before the clip.
    ``alpha`` / ``beta`` ((2,) or (P, 2)): the jitter C' = alpha C + beta of the rescaled concentrations; ``own_basis``: no rescale, and
    the tile is rebuilt with ``he`` itself."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        conc = concentrations64(x, he)
        if not own_basis:
            conc = conc * (np.asarray(tmc, dtype=np.float64).reshape(2) / np.asarray(max_c, dtype=np.float64).reshape(2))
        if alpha is not None:
            conc = np.asarray(alpha, dtype=np.float64) * conc + np.asarray(beta, dtype=np.float64)
        raw = rebuild64(conc, he if own_basis else sm)
    return {"out": np.clip(raw, 0.0, 255.0), "raw": raw}


def separation64(x: np.ndarray, he, max_c, sm, tmc) -> dict:
    """Stain separation with a given basis in float64: ``conc`` (P, 2) own-basis concentrations (normalised mode: times ``scale`` =
    tmc / maxC), ``own`` and ``normalised`` (P, 2, 3): the un-clamped H and E levels, stain i rebuilt from C_i alone with ``he`` / from
    C_i scale_i with ``sm``."""
    conc = concentrations64(x, he)
    he, sm = np.asarray(he, dtype=np.float64).reshape(3, 2), np.asarray(sm, dtype=np.float64).reshape(3, 2)
    scale = np.asarray(tmc, dtype=np.float64).reshape(2) / np.asarray(max_c, dtype=np.float64).reshape(2)
    own = np.stack([rebuild64(conc[:, s:s + 1], he[:, s:s + 1]) for s in range(2)], axis=1)
    normalised = np.stack([rebuild64(conc[:, s:s + 1] * scale[s], sm[:, s:s + 1]) for s in range(2)], axis=1)
    return {"conc": conc, "own": own, "normalised": normalised}


def _as_tile(x: np.ndarray) -> np.ndarray:
    """(P, 3) pixels as one (1, 3, 1, P) tile, what the restatements of tests/_deconv_numpy.py and tests/_luminosity_numpy.py take."""
    return np.ascontiguousarray(np.asarray(x).T).reshape(1, 3, 1, -1)


def _as_pixels(tile: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(tile.reshape(3, -1).T)


def basis_of(name: str) -> np.ndarray:
    """The (3, 3) float32 basis ``ColorDeconvolution(name)`` uses."""
    return stain_basis(name).numpy()


def deconv64(x32: np.ndarray, name: str) -> dict:
    """tests/_deconv_numpy.py on (P, 3) float32 unit pixels, float64 throughout: ``conc`` (P, 3); the un-clamped levels of apply with
    dn.ALPHA / dn.BETA (``apply``) and of apply rebuilt with the other basis (``target``); ``stains`` (P, 3 images, 3 channels)."""
    tile, basis = _as_tile(np.asarray(x32, dtype=F32)), basis_of(name)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out = {"conc": _as_pixels(dn.concentrations(tile, basis)),
               "apply": _as_pixels(dn.apply(tile, basis, alpha=[dn.ALPHA], beta=[dn.BETA], dtype=np.float64)),
               "target": _as_pixels(dn.apply(tile, basis, target=basis_of(OTHER_BASIS[name]), dtype=np.float64)),
               "stains": np.stack([_as_pixels(img) for img in dn.stain_images(tile, basis, dtype=np.float64)], axis=1)}
    return out


def luminosity64(x32: np.ndarray) -> dict:
    """tests/_luminosity_numpy.py's map on (P, 3) float32 unit pixels for the rows LUMINOSITY_Y, in float64, from its own functions (the
    CPU file holds clip(raw) to ln.standardize_unit bit for bit): ``raw`` (P, rows, 3) unit values BEFORE the clamp to [0, 1]; and which
    way every branch went: ``gamma_in`` (P, 3), ``f`` (P, 3), ``f_inv`` and ``gamma_out`` (P, rows, 3), ``clamp`` (P, rows): the
    min(100 L* / L_p, 100) took 100."""
    tile = _as_tile(np.asarray(x32, dtype=F32))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = ln.unit(tile)
        gamma_in = u > 0.04045
        xyz = np.einsum("ij,njhw->nihw", ln.RGB2XYZ, ln.linear(u)) / ln.WHITE
        cube = xyz > 0.008856
        f = ln.f_values(tile)
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        raw, f_inv, gamma_out, clamp = [], [], [], []
        for y_p in LUMINOSITY_Y:
            g = ln.gain(np.array([y_p]))[0][0]
            lifted = g * fy + (16.0 / 116.0) * (1.0 - g)
            fy2 = np.minimum(lifted, 1.0)
            f2 = np.stack([fy2 + (fx - fy), fy2, fy2 - (fy - fz)], axis=1)
            lin = np.einsum("ij,njhw->nihw", ln.XYZ2RGB, ln.f_inv(f2) * ln.WHITE)
            curve = lin > 0.0031308
            raw.append(_as_pixels(np.where(curve, 1.055 * _pow(curve, lin, 1.0 / 2.4) - 0.055, 12.92 * lin)))
            f_inv.append(_as_pixels(f2 > 0.2068966))
            gamma_out.append(_as_pixels(curve))
            clamp.append((lifted >= 1.0).reshape(-1))
    return {"raw": np.stack(raw, axis=1), "gamma_in": _as_pixels(gamma_in), "f": _as_pixels(cube), "f_inv": np.stack(f_inv, axis=1), "gamma_out": np.stack(gamma_out, axis=1),
            "clamp": np.stack(clamp, axis=1)}


def grey_levels(x32: np.ndarray) -> np.ndarray:
    """The grey-level gate of histogram matching in float32, exactly ``so.images_to_uint8`` -- exact arithmetic, so no tolerance anywhere.
    The reference's cast of a NaN is undefined; the library's rule is bin 0 (fmaxf(NaN, 0) = 0), restated here by gating 0 in its place.
    +Inf -> 255 and -Inf -> 0 are the reference's own clamp."""
    x32 = np.asarray(x32, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return so.images_to_uint8(np.where(np.isnan(x32), F32(0), x32))[0]


def near_integer(raw_levels: np.ndarray, bound: float) -> np.ndarray:
    """uint8 outputs: the elements that may come out one level off -- the float64 value (on the 0-255 scale, BEFORE the clip) lies within
    ``bound`` of an integer of 0..255.  A saturated element, further than the bound outside 0..255, is not among them: it has to come out
    as exactly 0 or 255 (its clipped value IS an integer, so counting it as "near" would only loosen the rule there)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(raw_levels - np.rint(raw_levels)) <= bound) & (raw_levels >= -bound) & (raw_levels <= 255.0 + bound)


def half_ulp(ref: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """Half a unit in the last place of ``dtype`` (bfloat16 / float16) at the reference value: the rounding of a value to that type."""
    bits, e_min = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    e = np.where(np.isfinite(e), np.maximum(e, e_min), e_min)
    return 0.5 * np.exp2(e - bits)


def _in_slices(fn, x: np.ndarray) -> dict:
    out: dict[str, np.ndarray] = {}
    for s in range(0, len(x), SLICE):
        part = fn(x[s:s + SLICE])
        part = part if isinstance(part, dict) else {"out": part}
        for key, value in part.items():
            if key not in out:
                out[key] = np.empty((len(x),) + value.shape[1:], dtype=value.dtype)
            out[key][s:s + SLICE] = value
    return out


# ------------------------------------------------------------------------------------------------ the fixed statistics
@lru_cache(maxsize=None)
def statistics() -> dict:
    """Reinhard: source = so.reinhard_fit of he_batch(4, 128, 128, seed0=900), reference = so.reinhard_fit of reference_tile(128, 128).
    Macenko: source = so.macenko_tile_params(signs="positive_sum") of he_batch(1, 128, 128, seed0=900), target = the real-tissue fixture's."""
    mean, std = so.reinhard_fit(synth.he_batch(4, 128, 128, seed0=900).numpy())
    ref_mean, ref_std = so.reinhard_fit(synth.reference_tile(128, 128).numpy())
    od = so.optical_density(so.to_unit_float(synth.he_batch(1, 128, 128, seed0=900).numpy()))
    p = so.macenko_tile_params(od[0], signs="positive_sum")
    with np.load(GOLDEN / "g11_real_tissue.npz", allow_pickle=False) as g:
        sm, tmc = g["stain_matrix"].astype(F32), g["target_max_conc"].astype(F32)
    out = {"mean": mean, "std": std, "ref_mean": ref_mean, "ref_std": ref_std, "he": p["he"].astype(F32), "max_c": p["max_c"].astype(F32), "sm": sm, "tmc": tmc}
    assert all(np.isfinite(v).all() for v in out.values()) and (out["max_c"] != 0).all() and (out["std"] > 0).all()
    return out


# ------------------------------------------------------------------------------------------------ sets and layouts
class Layout:
    def __init__(self, name: str, n: int, h: int, w: int, index: np.ndarray):
        assert index.shape == (n * h * w,)
        self.name, self.n, self.h, self.w, self.index = name, n, h, w, index

    @property
    def packs(self) -> bool:
        return (self.h * self.w) % 16 == 0


def _layout(name: str, h: int, w: int, blocks: list[np.ndarray], pad: int, seed: int) -> Layout:
    """Every block of pixel indices gets whole tiles of its own, permuted inside them and filled up with the pad pixel."""
    rng = np.random.default_rng(seed)
    parts = []
    for block in blocks:
        tiles = -(-len(block) // (h * w))
        full = np.full(tiles * h * w, pad, dtype=np.int64)
        full[:len(block)] = block
        parts.append(rng.permutation(full))
    index = np.concatenate(parts)
    return Layout(name, len(index) // (h * w), h, w, index)


class Sweep:
    """``pixels``: (P, 3) torch tensor of the element type, the last one the 0.5-grey pad; ``layouts``: {"packs": ..., "odd": ...}."""

    def __init__(self, name: str, pixels: torch.Tensor, layouts: dict[str, Layout], triples: np.ndarray | None = None):
        self.name, self.pixels, self.dtype, self.layouts = name, pixels, pixels.dtype, layouts
        self.triples = np.zeros(len(pixels), dtype=bool) if triples is None else triples      # (P,): the random triples of set C
        self._jitter: dict = {}
        self._deconv: dict = {}

    def __repr__(self) -> str:
        return f"Sweep({self.name}, {len(self.pixels)} pixels)"

    @cached_property
    def x32(self) -> np.ndarray:
        """(P, 3) float32 unit values: what every kernel makes of an element (u8 / 255 as the oracle's gate; bf16 / f16 -> float32 is exact)."""
        return so.to_unit_float(self.pixels.numpy()) if self.dtype in (torch.uint8, torch.float32) else self.pixels.float().numpy()

    @cached_property
    def finite(self) -> np.ndarray:
        return np.isfinite(self.x32).all(axis=1)

    def _within(self, lo: float, hi: float) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return ((self.x32 >= F32(lo)) & (self.x32 <= F32(hi))).all(axis=1)

    @cached_property
    def reinhard_domain(self) -> np.ndarray:
        """Every member in [-1, 2]; for the random triples of set C every member in [-1/4, 5/4].  Narrowed there, not the bound widened: a
        triple with one member near 2 and another below 0 has a dark, out-of-gamut channel, where the output gamma's slope of 12.92 meets
        the cancellation of the float32 colour matrices, and the float32 ORACLE itself is 4.1e-5 from float64 on [-1, 2]^3 (2.3e-5 on
        [-1/2, 3/2]^3, 1.3e-5 on [-1/4, 5/4]^3; 1.1e-5 on [0, 1]^3) -- more than the quarter of the bound it may take
        (tests/test_value_sweep_cpu.py).  The grey axis and the channel sweeps keep [-1, 2]."""
        return self._within(-1.0, 2.0) & (~self.triples | self._within(*TRIPLE_DOMAIN))

    @cached_property
    def macenko_domain(self) -> np.ndarray:
        return self._within(-1.0 / 512.0, 2.0)

    # ---- float64 references, once per set
    @cached_property
    def reinhard(self) -> dict:
        st = statistics()
        return _in_slices(lambda x: reinhard64(x, st["mean"], st["std"], st["ref_mean"], st["ref_std"]), self.x32)

    @cached_property
    def macenko(self) -> dict:
        st = statistics()
        return _in_slices(lambda x: macenko64(x, st["he"], st["max_c"], st["sm"], st["tmc"]), self.x32)

    @cached_property
    def luminosity_domain(self) -> np.ndarray:
        """Every member in [0, 1], where the float32 oracle's round trip is within a quarter of the bound of float64 at the three gains
        (tests/test_value_sweep_cpu.py prints the figures).  Not widened: nothing outside [0, 1] has been measured at the gain 3.33."""
        return self._within(0.0, 1.0)

    @cached_property
    def separation(self) -> dict:
        st = statistics()
        return _in_slices(lambda x: separation64(x, st["he"], st["max_c"], st["sm"], st["tmc"]), self.x32)

    def jitter(self, layout: "Layout", own_basis: bool, shift: int = 0) -> dict:
        """macenko64 with C' = alpha C + beta over the LAYOUT's pixels (the factors are per tile: tile t takes JITTER[(t + shift) % 3];
        :func:`row_shifts` gives a layout of fewer tiles than pairs one call per pair), normalised or in the source's own basis: ``raw``
        (N, 3, H, W) float64 before the clip, ``alpha`` / ``beta`` (N, 2) float32, ``pair`` (N,) the index into JITTER.  Once per layout."""
        key = (layout.name, bool(own_basis), shift)
        if key not in self._jitter:
            st = statistics()
            which = (np.arange(layout.n) + shift) % len(JITTER)
            pairs = np.asarray(JITTER, dtype=np.float64)[which]      # (N, 2 (alpha, beta), 2 (H, E))
            per_pixel = np.repeat(pairs, layout.h * layout.w, axis=0)
            x = self.x32[layout.index]
            raw = np.concatenate([macenko64(x[s:s + SLICE], st["he"], st["max_c"], st["sm"], st["tmc"], alpha=per_pixel[s:s + SLICE, 0], beta=per_pixel[s:s + SLICE, 1],
                                            own_basis=own_basis)["raw"] for s in range(0, len(x), SLICE)])
            raw = np.ascontiguousarray(raw.reshape(layout.n, layout.h, layout.w, 3).transpose(0, 3, 1, 2))
            self._jitter[key] = {"raw": raw, "alpha": pairs[:, 0].astype(F32), "beta": pairs[:, 1].astype(F32), "pair": which}
        return self._jitter[key]

    def deconv(self, name: str) -> dict:
        if name not in self._deconv:
            self._deconv[name] = _in_slices(lambda x: deconv64(x, name), self.x32)
        return self._deconv[name]

    @cached_property
    def luminosity(self) -> dict:
        return _in_slices(luminosity64, self.x32)

    @cached_property
    def levels(self) -> np.ndarray:
        """(P, 3) uint8: the grey level of every member (:func:`grey_levels`)."""
        return grey_levels(self.x32)

    @property
    def lightness(self) -> np.ndarray:
        """(P,) float64 L on the oracle's 0..255 scale: the rule is L < 255 * threshold (L* / 100 < threshold)."""
        return self.reinhard["lab"][:, 0]

    def rule(self, threshold: float, band: float) -> tuple[np.ndarray, np.ndarray]:
        """(tissue, decided) per pixel by the float64 rule: a NaN pixel is background and decided; a pixel whose float64 L is NaN without a
        NaN member (+Inf and -Inf in one pixel) and a pixel within ``band`` of the cut are not decided."""
        lum, cut = self.lightness, 255.0 * threshold
        with np.errstate(invalid="ignore"):
            tissue = lum < cut
            decided = np.abs(lum - cut) > band
        has_nan = np.isnan(self.x32).any(axis=1)
        return tissue & ~has_nan, decided | has_nan

    # ---- tiles
    def index(self, layout: Layout, replace: np.ndarray | None = None) -> np.ndarray:
        """The pixel of the list at every position of the layout; the pixels of ``replace`` ((P,) bool) replaced by the 0.5-grey pad."""
        return layout.index if replace is None else np.where(replace[layout.index], len(self.pixels) - 1, layout.index)

    def images(self, layout: Layout, *, channels_last: bool = False, replace: np.ndarray | None = None) -> torch.Tensor:
        """The layout's tiles, NCHW (or NHWC)."""
        nhwc = self.pixels[torch.from_numpy(self.index(layout, replace))].view(layout.n, layout.h, layout.w, 3)
        return nhwc.contiguous() if channels_last else nhwc.permute(0, 3, 1, 2).contiguous()

    def spread(self, layout: Layout, per_pixel: np.ndarray, replace: np.ndarray | None = None) -> np.ndarray:
        """A per-pixel array (P,) or (P, K) carried to the layout: (N, H, W) or (N, K, H, W)."""
        got = per_pixel[self.index(layout, replace)]
        if got.ndim == 1:
            return got.reshape(layout.n, layout.h, layout.w)
        return np.ascontiguousarray(got.reshape(layout.n, layout.h, layout.w, got.shape[1]).transpose(0, 3, 1, 2))


def _both_layouts(blocks: list[np.ndarray], pad: int, packs: tuple[int, int], odd: tuple[int, int], seed: int) -> dict[str, Layout]:
    assert (packs[0] * packs[1]) % 16 == 0 and odd[1] % 2 == 1 and (odd[0] * odd[1]) % 2 == 1
    return {"packs": _layout("packs", *packs, blocks, pad, seed), "odd": _layout("odd", *odd, [np.concatenate(blocks)], pad, seed + 1)}


@lru_cache(maxsize=None)
def set_a() -> Sweep:
    """All 2^24 uint8 colours; 0.5 grey is level 128 (an element of the list already)."""
    i = torch.arange(1 << 24, dtype=torch.int32)
    colours = torch.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], dim=1).to(torch.uint8)
    pixels = torch.cat([colours, torch.tensor([[128, 128, 128]], dtype=torch.uint8)])
    return Sweep("A_u8_all_colours", pixels, _both_layouts([np.arange(1 << 24)], 1 << 24, (4096, 4096), (4099, 4095), 11))


@lru_cache(maxsize=None)
def set_a_small() -> Sweep:
    """uint8 through the single-element path: every level in every channel -- the grey axis and the six channel sweeps of
    :func:`_axis_and_sweeps`, the fixed members as levels -- and 2^16 seeded colours, in an odd layout ONLY (255 x 257 tiles: odd W, odd
    H * W, four work items of 16 384 pixels each).  Set A then needs its 2^24 colours in the pack layout alone."""
    levels = torch.arange(256, dtype=torch.uint8)
    parts = [levels[:, None].expand(-1, 3)]
    for fixed in FIXED:
        for c in range(3):
            px = torch.tensor([round(255 * v) for v in fixed], dtype=torch.uint8).repeat(256, 1)
            px[:, c] = levels
            parts.append(px)
    colours = torch.from_numpy(np.random.default_rng(2031).integers(0, 256, size=(1 << 16, 3), dtype=np.uint8))
    pixels = torch.cat(parts + [colours, torch.tensor([[128, 128, 128]], dtype=torch.uint8)])
    h, w = 255, 257
    assert w % 2 == 1 and (h * w) % 2 == 1 and h * w >= 2 * 16384
    return Sweep("A_small_u8", pixels, {"odd": _layout("odd", h, w, [np.arange(len(pixels) - 1)], len(pixels) - 1, 12)})


def _axis_and_sweeps(values: torch.Tensor) -> torch.Tensor:
    """(7 V, 3): the grey axis (v, v, v), then every channel swept with the other two fixed at FIXED[0] and at FIXED[1]."""
    parts = [values[:, None].expand(-1, 3)]
    for fixed in FIXED:
        for c in range(3):
            px = torch.tensor(fixed, dtype=torch.float32).to(values.dtype).repeat(len(values), 1)
            px[:, c] = values
            parts.append(px)
    return torch.cat(parts)


@lru_cache(maxsize=None)
def set_b(dtype: torch.dtype) -> Sweep:
    """Every 16-bit pattern of bfloat16 / float16 (65 536, NaN payloads and both infinities included)."""
    patterns = (torch.arange(1 << 16, dtype=torch.int32) - (1 << 15)).to(torch.int16).view(dtype)      # every int16 is a pattern
    pixels = torch.cat([_axis_and_sweeps(patterns), torch.full((1, 3), 0.5, dtype=dtype)])
    name = {torch.bfloat16: "B_bf16_all_patterns", torch.float16: "B_f16_all_patterns"}[dtype]
    return Sweep(name, pixels, _both_layouts([np.arange(len(pixels) - 1)], len(pixels) - 1, (256, 256), (255, 257), 23))


def _neighbours(centre: np.ndarray, reach: int) -> np.ndarray:
    """The float32 values up to ``reach`` steps either side of every centre (through zero and the denormals where that is where they lie)."""
    centre = np.asarray(centre, dtype=F32).reshape(-1)
    out, up, down = [centre], centre, centre
    for _ in range(reach):
        up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
        out += [up, down]
    return np.concatenate(out)


def grey_crossings() -> np.ndarray:
    """The grey value v at which X/Xn, Y and Z/Zn of (v, v, v) cross 0.008856, solved in float64 (all three lie on the power branch of the
    input gamma: v ~ 0.09)."""
    lin = 0.008856 * _D65 / _RGB2XYZ.sum(axis=1)
    v = 1.055 * lin ** (1.0 / 2.4) - 0.055
    assert (v > 0.04045).all()
    return v


@lru_cache(maxsize=None)
def c_values() -> tuple[np.ndarray, np.ndarray]:
    """(finite values, the non-finite group) of set C, float32."""
    tiny = np.finfo(F32)
    lattice = np.arange(256, dtype=F32) / F32(255.0)
    rng = np.random.default_rng(2027)
    special = np.array([0.0, -0.0, tiny.smallest_subnormal, np.nextafter(tiny.tiny, F32(0)), tiny.tiny, np.nextafter(F32(1), F32(0)), 1.0, np.nextafter(F32(1), F32(2)),
                        2.0, -1.0 / 512.0, -1.0], dtype=F32)
    finite = np.concatenate([_neighbours(lattice, 2), _neighbours(F32(0.04045), 33), _neighbours(grey_crossings().astype(F32), 33), special,
                             rng.random(1 << 20, dtype=F32), (rng.random(1 << 18, dtype=F32) * F32(3.0) - F32(1.0)).astype(F32)])
    group = np.array([np.inf, -np.inf, np.nan, tiny.max, -tiny.max], dtype=F32)
    return finite, group


LATTICE_TILES = 2      # tiles of set C's pack layout that hold k / 255 values only (they pass the 8-bit code gates)


@lru_cache(maxsize=None)
def set_c() -> Sweep:
    finite, group = c_values()
    rng = np.random.default_rng(2028)
    lattice = np.arange(256, dtype=F32) / F32(255.0)
    # (lattice values in every member: the grey axis and random lattice triples -- the fixed members of a channel sweep are not grey levels)
    lattice_px = np.concatenate([np.repeat(lattice[:, None], 3, axis=1), lattice[rng.integers(0, 256, size=(LATTICE_TILES * 512 * 512 - 256, 3))]])
    triples = finite[rng.integers(0, len(finite), size=(1 << 20, 3))]
    mixed = finite[rng.integers(0, len(finite), size=(1 << 12, 3))]      # random triples with one member of the non-finite group
    mixed[np.arange(len(mixed)), rng.integers(0, 3, size=len(mixed))] = group[rng.integers(0, len(group), size=len(mixed))]
    rest = np.concatenate([_axis_and_sweeps(torch.from_numpy(finite)).numpy(), triples, _axis_and_sweeps(torch.from_numpy(group)).numpy(), mixed])
    pixels = torch.from_numpy(np.concatenate([lattice_px, rest, np.full((1, 3), 0.5, dtype=F32)]).astype(F32))
    blocks = [np.arange(len(lattice_px)), len(lattice_px) + np.arange(len(rest))]
    triples = np.zeros(len(pixels), dtype=bool)
    first = len(lattice_px) + 7 * len(finite)
    triples[first:first + (1 << 20)] = True
    return Sweep("C_f32", pixels, _both_layouts(blocks, len(pixels) - 1, (512, 512), (511, 513), 37), triples)


def stain_layouts(sweep: Sweep) -> list[Layout]:
    """The layouts of the stain sweeps: set A's 2^24 colours run ONCE, in the pack layout (A_small covers the single-element path)."""
    return [sweep.layouts["packs"]] if sweep.name.startswith("A_u8") else list(sweep.layouts.values())


def row_shifts(layout: Layout, rows: int) -> range:
    """Per-tile rows are dealt in turn, tile t taking row (t + shift) % rows: one shift where the layout has a tile for every row, every
    shift where it has not (set A's pack layout is ONE tile)."""
    return range(1) if layout.n >= rows else range(rows)


@lru_cache(maxsize=None)
def concentration_set() -> Sweep:
    """float32 (P, 3) CONCENTRATIONS for ColorDeconvolution.combine, which need not come out of a separation: the concentrations of set
    C's in-domain pixels under ``hed`` (rounded to float32) -- without C's two lattice-only tiles: combine(separate(k / 255)) is the
    integer k + 1, and with those 2^19 pixels 15.3 % of the uint8 reference of ``hed`` lies within the bound of an integer, over the cap
    of tests/test_value_sweep_cpu.py; the lattice and its neighbours stay, in the axis and the sweeps of set C --; the grey axis and one-stain sweeps over [-4, 12] (the other two fixed at
    (0.5, 0.2, 0.1) and at (1.5, 1.0, 0.3)); 2^18 uniform triples in [-2, 6)^3; and +-Inf, NaN, +-FLT_MAX, +-1e30 as a block of its
    own.  The pad is (0.5, 0.5, 0.5).  ``combine_domain``: every member finite with |C| <= 12."""
    c = set_c()
    rng = np.random.default_rng(2032)
    beside_lattice = np.arange(len(c.pixels)) >= LATTICE_TILES * 512 * 512      # (not the lattice tiles: see the docstring)
    with np.errstate(over="ignore", invalid="ignore"):
        separated = c.deconv("hed")["conc"][c.macenko_domain & beside_lattice].astype(F32)
    line = np.concatenate([np.linspace(-4.0, 12.0, 1 << 14, dtype=np.float64).astype(F32), _neighbours(np.array([0.0, -0.0, 12.0, -4.0], dtype=F32), 2)])
    swept = [np.repeat(line[:, None], 3, axis=1)]
    for fixed in ((0.5, 0.2, 0.1), (1.5, 1.0, 0.3)):
        for s in range(3):
            px = np.tile(np.asarray(fixed, dtype=F32), (len(line), 1))
            px[:, s] = line
            swept.append(px)
    uniform = (rng.random((1 << 18, 3), dtype=F32) * F32(8.0) - F32(2.0)).astype(F32)
    tiny = np.finfo(F32)
    group = np.array([np.inf, -np.inf, np.nan, tiny.max, -tiny.max, 1e30, -1e30], dtype=F32)
    wild = uniform[: 1 << 12].copy()
    wild[np.arange(len(wild)), rng.integers(0, 3, size=len(wild))] = group[rng.integers(0, len(group), size=len(wild))]
    wild = np.concatenate([np.repeat(group[:, None], 3, axis=1), wild])
    finite = np.concatenate([separated] + swept + [uniform])
    pixels = torch.from_numpy(np.concatenate([finite, wild, np.full((1, 3), 0.5, dtype=F32)]).astype(F32))
    blocks = [np.arange(len(finite)), len(finite) + np.arange(len(wild))]
    return Sweep("K_f32_concentrations", pixels, _both_layouts(blocks, len(pixels) - 1, (512, 512), (511, 513), 41))


def combine_domain(sweep: Sweep) -> np.ndarray:
    c = sweep.pixels.numpy()
    with np.errstate(invalid="ignore"):
        return (np.isfinite(c) & (np.abs(c) <= F32(COMBINE_DOMAIN))).all(axis=1)


@lru_cache(maxsize=None)
def combine64(name: str) -> np.ndarray:
    """(P, 3) float64: dn.combine of the concentration set with the basis ``name``, un-clamped levels."""
    c = concentration_set().pixels.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        return _in_slices(lambda part: _as_pixels(dn.combine(_as_tile(part), basis_of(name), dtype=np.float64)), c)["out"]


def float_sets() -> list[Sweep]:
    return [set_b(torch.bfloat16), set_b(torch.float16), set_c()]


def all_sets() -> list[Sweep]:
    return [set_a()] + float_sets()


# ------------------------------------------------------------------------------------------------ the tiles of the 8-bit code gates
GATE_SHAPE = (16, 256, 256)            # 2^20 pixels, H * W % 4 == 0: the smallest batch the coded paths of both transforms take
GATE_MOVED_PIXEL = (64, 64, 64)        # grey levels of the pixel that holds a moved element: 64 / 255 lies just above 1 / 4, where one ulp is relatively
                                       # largest -- of nine pixels tried against a tolerance gate, the one that showed it at all three spots in both transforms
_PACKS = GATE_SHAPE[1] * GATE_SHAPE[2] // 4
GATE_SPOTS = {"first pack": (0, 0), "middle lane": (1, 4 * (_PACKS // 2 + 29) + 2), "last pack": (2, 4 * _PACKS - 1)}      # (channel, pixel of the tile)


@lru_cache(maxsize=None)
def gate_tiles() -> tuple[torch.Tensor, dict[str, int]]:
    """((16, 3, 256, 256) float32, {what a tile holds: its index}).  Every tile starts as an H&E tile of k / 255 values (a well-posed Macenko
    estimate), which passes the code gates.  Then, with every value kept inside [0, 1]:

    * ``all up`` / ``all down``: EVERY element one ulp above / below its grey level (at 1 and at 0: the one neighbour inside the range);
    * ``all mixed``: every element one ulp off, the direction drawn per element;
    * ``<spot> up`` / ``<spot> down``: grey levels but for ONE element, moved by one ulp -- in the first pack, in the last pack and in a
      lane in the middle of a wave (GATE_SPOTS), the pixel around it set to GATE_MOVED_PIXEL;
    * ``<spot> -0``: grey levels but for one element that is -0.0 where its pixel holds level 0;
    * ``levels ...``: untouched tiles (first, between and last), which the gates pass.

    A gate has to fail every tile but the ``levels`` ones: its comparison is of BITS.  One that took the nearest level, or compared values
    within a tolerance, would code a moved tile and hand table[k] to elements that hold k / 255 +- 1 ulp."""
    n, h, w = GATE_SHAPE
    x = synth.as_dtype(synth.he_batch(n, h, w, seed0=4700), torch.float32).numpy().copy()
    lattice = np.arange(256, dtype=F32) / F32(255.0)
    assert np.isin(x, lattice).all()
    up = np.where(x < 1, np.nextafter(x, F32(2)), np.nextafter(x, F32(0)))
    down = np.where(x > 0, np.nextafter(x, F32(-1)), np.nextafter(x, F32(1)))
    tiles: dict[str, int] = {"levels first": 0, "all up": 1, "all down": 2, "all mixed": 3, "levels between": 7, "levels next to last": 14, "levels last": 15}
    x[1], x[2] = up[1], down[2]
    x[3] = np.where(np.random.default_rng(2029).random(x[3].shape) < 0.5, up[3], down[3])
    slots = iter((4, 5, 6, 8, 9, 10, 11, 12, 13))
    for kind in ("up", "down", "-0"):
        for spot, (c, p) in GATE_SPOTS.items():
            t = next(slots)
            flat = x[t].reshape(3, h * w)
            flat[:, p] = lattice[list(GATE_MOVED_PIXEL)]
            if kind == "-0":
                flat[c, p] = F32(-0.0)
            else:
                flat[c, p] = np.nextafter(flat[c, p], F32(2 if kind == "up" else -1))
            tiles[f"{spot} {kind}"] = t
    assert x.min() >= 0 and x.max() <= 1 and sorted(tiles.values()) == list(range(n))
    return torch.from_numpy(x), tiles


def monotone_tables(seed: int = 5) -> np.ndarray:
    """(1, 3, 256) float32: a seeded non-decreasing table per channel with values in 0..255 (a foreign source for HistogramMatching.apply)."""
    rng = np.random.default_rng(seed)
    steps = rng.random((3, 256)) ** 3
    table = np.cumsum(steps, axis=1)
    return (255.0 * (table - table[:, :1]) / (table[:, -1:] - table[:, :1])).astype(F32)[None]
