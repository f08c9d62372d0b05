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

    gate_tiles()  float32 tiles for the 8-bit code gates, which mark WHOLE tiles: grey levels, every element one ulp off, one element off.

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
from stainx_amd import synth

F32 = np.float32
SLICE = 1 << 20
GOLDEN = Path(__file__).resolve().parent / "golden"
FIXED = ((0.85, 0.55, 0.75), (0.3, 0.2, 0.5))      # the other two channels of a one-channel sweep
THRESHOLDS = (0.5, 0.8, 0.9)                       # luminosity thresholds of the rule tests
REINHARD_TOL = 1e-4                                # the project's parity bound on [0, 1] (tests/test_siblings_gpu.py, test_per_tile_gpu.py)
TRIPLE_DOMAIN = (-0.25, 1.25)                      # the Reinhard domain of set C's random triples (Sweep.reinhard_domain says why)
MIN_BRANCH_PIXELS = 1000                           # coverage: in-domain pixels on either side of every branch, per float set

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


def macenko64(x: np.ndarray, he, max_c, sm, tmc) -> dict:
    """The tail of the Macenko transform with a GIVEN (HE, maxC, SM, targetMaxC) (oracle/stain_oracle.py:58, 117, 162-164) in float64:
    OD = -log((255 x + 1) / 240), least squares, rescale, 240 exp(-OD'), clipped to 0..255.  (P, 3) in; ``out`` (P, 3), ``raw`` before the clip."""
    he, sm = np.asarray(he, dtype=np.float64).reshape(3, 2), np.asarray(sm, dtype=np.float64).reshape(3, 2)
    scale = np.asarray(tmc, dtype=np.float64).reshape(2) / np.asarray(max_c, dtype=np.float64).reshape(2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        od = -np.log((np.asarray(x, dtype=np.float64) * 255.0 + 1.0) / 240.0)
        conc = np.linalg.lstsq(he, od.T, rcond=None)[0]      # (2, P)
        od_new = (sm @ (conc * scale[:, None])).T
        raw = 240.0 * np.exp(-od_new)
    return {"out": np.clip(raw, 0.0, 255.0), "raw": raw}


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
        """A per-pixel array (P,) or (P, 3) carried to the layout: (N, H, W) or (N, 3, H, W)."""
        got = per_pixel[self.index(layout, replace)]
        if got.ndim == 1:
            return got.reshape(layout.n, layout.h, layout.w)
        return np.ascontiguousarray(got.reshape(layout.n, layout.h, layout.w, 3).transpose(0, 3, 1, 2))


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
