"""HSV colour augmentation on the GPU, through the C ABI (sx_hsv_apply, sx_hsv_apply_masked) and through ``adjust_hsv`` / ``HSVAugment``.

The yardstick is tests/_hsv_numpy.py: the pixel rule in float64 on the float32 values the kernel reads, evaluated ONCE per pixel list and
row and carried to the layouts through their index.  Bounds (on [0, 1] unless levels are named):
  float outputs                   1e-4, the project's bound for its other colour-space maps (REINHARD_TOL, LUMINOSITY_TOL);
  bf16 / f16 outputs              plus half a unit in the last place of the type at 1: 2^-9 / 2^-12;
  uint8 output                    |out - level64| <= 0.5 + 1e-3 levels for EVERY element (rounding to nearest; a tie within the float32
                                  arithmetic's 1e-3 may go either way);
  uint8 tiles, float output       the level is quantised to 8 bits first (the output rule), so the same band holds for 255 x out (x 1
                                  without the / 255), widened by the half unit of the output type where the / 255 is rounded to it.
The identity row needs no reference: all 2^24 uint8 colours come back ``torch.equal``.  Copies (NaN members, non-finite rows, masked-out
pixels) are exact: the bits of the background rule.  ``SX_MACENKO_NORMALIZE_0_1`` on float tiles is held to an exact relation (the level
output divided by 255 by the output rule), not to a bound: a 16-bit tile is rounded twice there.

Measured on an MI355X (the figures this file prints; DESIGN.md 4r quotes them): uint8 output 0.50002 levels, float32 / float64 1.23e-6,
float16 2.452e-4, bfloat16 1.961e-3 (the last two are the rounding of a level to the type), uint8 tiles with ``/ 255`` to bf16 0.99609 and to
f16 0.56120 levels."""
from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

from stainx_amd import HSVAugment, _native, adjust_hsv, tissue_mask
from tests import _hsv_numpy as hn
from tests import _value_sweep as vs

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAND = 0.5 + 1e-3
HALF_ULP_AT_1 = {torch.bfloat16: 2.0**-9, torch.float16: 2.0**-12, torch.float32: 2.0**-25, torch.float64: 0.0}
PACKS, ODD = (144, 128), (33, 31)      # H * W % 16 == 0 and more than a work item's pixels (16 384 for uint8: a second, partial work item); odd W, odd H * W
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64)
CL, UNIT, CLASSIC = _native.MACENKO_CHANNELS_LAST, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_CLASSIC
OUT_FLAG = {torch.bfloat16: _native.MACENKO_OUT_BF16, torch.float16: _native.MACENKO_OUT_F16}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def lib():
    return _native.require()


# ------------------------------------------------------------------ the pixel lists and their references
@lru_cache(maxsize=None)
def pixels_of(dtype: torch.dtype) -> torch.Tensor:
    """(P, 3) of the element type, the last one the 0.5-grey pad.
    uint8: every level in every channel (set A_small: the grey axis, six channel sweeps, 2^16 seeded colours) and every pixel with two
    equal channels (3 x 256^2: the sector boundaries and the ties of the max); float32 / float64: the k / 255 lattice with its +-1 ulp
    neighbours as grey axis and channel sweeps, 2^16 triples of set C's seeded uniforms in [0, 1), 2^14 of its uniforms in [-1, 2], and
    triples with one member of set C's non-finite group; bfloat16 / float16: set B, every 16-bit pattern as grey axis and channel sweeps."""
    if dtype == torch.uint8:
        a, b = torch.meshgrid(torch.arange(256, dtype=torch.uint8), torch.arange(256, dtype=torch.uint8), indexing="ij")
        a, b = a.reshape(-1), b.reshape(-1)
        equal = torch.cat([torch.stack([a, a, b], 1), torch.stack([a, b, a], 1), torch.stack([b, a, a], 1)])
        small = vs.set_a_small().pixels
        return torch.cat([small[:-1], equal, small[-1:]])
    if dtype in (torch.bfloat16, torch.float16):
        return vs.set_b(dtype).pixels
    finite, group = vs.c_values()
    unit, wide = finite[-((1 << 20) + (1 << 18)):-(1 << 18)], finite[-(1 << 18):]      # (c_values: the last two blocks are the seeded uniforms)
    lattice = vs._neighbours(np.arange(256, dtype=np.float32) / np.float32(255.0), 1)
    rng = np.random.default_rng(59)
    mixed = unit[:3 << 10].reshape(-1, 3).copy()
    mixed[np.arange(len(mixed)), rng.integers(0, 3, size=len(mixed))] = group[rng.integers(0, len(group), size=len(mixed))]
    parts = [vs._axis_and_sweeps(torch.from_numpy(lattice)).numpy(), unit[3 << 10:(3 << 10) + (3 << 16)].reshape(-1, 3), wide[:3 << 14].reshape(-1, 3), mixed,
             np.full((1, 3), 0.5, dtype=np.float32)]
    return torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(dtype)


@lru_cache(maxsize=None)
def reference(dtype: torch.dtype, row: tuple) -> tuple[np.ndarray, np.ndarray]:
    """``(level64 (P, 3), copied (P,))`` of the pixel list under ``row``; float64 tiles hold float32 values, read as float32 by the kernel."""
    return hn.levels64(hn.input_levels(pixels_of(dtype)), row)


@lru_cache(maxsize=None)
def index_of(dtype: torch.dtype, shape: tuple) -> np.ndarray:
    """(N, H, W) indices into the pixel list: every pixel once, in a seeded permutation, filled up with the pad."""
    count = len(pixels_of(dtype))
    per = shape[0] * shape[1]
    tiles = -(-count // per)
    index = np.full(tiles * per, count - 1, dtype=np.int64)
    index[:count] = np.arange(count)
    return np.random.default_rng(97 + per).permutation(index).reshape(tiles, *shape)


def images_of(dtype: torch.dtype, shape: tuple, channels_last: bool, dev) -> torch.Tensor:
    nhwc = pixels_of(dtype)[torch.from_numpy(index_of(dtype, shape))]
    return (nhwc if channels_last else nhwc.permute(0, 3, 1, 2)).contiguous().to(dev)


def as_pixels(out: torch.Tensor, channels_last: bool) -> torch.Tensor:
    return (out if channels_last else out.permute(0, 2, 3, 1)).reshape(-1, 3).cpu()


# ------------------------------------------------------------------ the raw call
def out_dtype_of(x: torch.Tensor, flags: int) -> torch.dtype:
    if x.dtype == torch.uint8:
        for dtype, flag in OUT_FLAG.items():
            if flags & flag:
                return dtype
        return torch.float32 if flags & UNIT else torch.uint8
    return x.dtype


def raw(lib, x: torch.Tensor, rows: torch.Tensor, flags: int = 0, mask: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """sx_hsv_apply / sx_hsv_apply_masked on the current stream; ``rows``: (R, 5) float32 on the device."""
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if flags & CL else (x.shape[0], x.shape[2], x.shape[3])
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype_of(x, flags), device=x.device)
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == 5
    stream = _native.stream_ptr(x.device)
    if mask is None:
        rc = lib.sx_hsv_apply(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, rows.data_ptr(), rows.shape[0], flags, stream)
    else:
        rc = lib.sx_hsv_apply_masked(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, rows.data_ptr(), rows.shape[0], mask.data_ptr(), flags, stream)
    assert rc == 0, _native.last_error(lib)
    return out


def row_tensor(rows, dev) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 5)


def off_by_one(t: torch.Tensor) -> torch.Tensor:
    """The same values one element off a 16-byte address (torch allocations are 256-byte aligned)."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


# ------------------------------------------------------------------ identity: all 2^24 colours, exact
def test_identity_row_returns_all_uint8_colours(dev, lib):
    sweep = vs.set_a()
    x = sweep.images(sweep.layouts["packs"]).to(dev)      # (1, 3, 4096, 4096)
    identity = row_tensor(hn.IDENTITY, dev)
    assert torch.equal(raw(lib, x, identity), x)
    assert torch.equal(adjust_hsv(x, identity[0]), x)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(raw(lib, nhwc, identity, CL), nhwc)
    got = raw(lib, x, identity, UNIT)      # the 8-bit level, rounded, then / 255 in float32 (the IEEE quotient: divided on the CPU, a device division by a scalar may be a product)
    assert torch.equal(got.cpu(), x.cpu().float() / 255.0)


# ------------------------------------------------------------------ against the float64 restatement
def check_levels(out: torch.Tensor, in_dtype: torch.dtype, unit: bool, level: np.ndarray, copied: np.ndarray, what) -> float:
    """``out``: (P', 3) on the CPU; ``level`` / ``copied``: the reference at the same pixels.  Prints the figure, then asserts."""
    got = out.to(torch.float64).numpy()
    assert np.isfinite(got).all(), what
    if in_dtype == torch.uint8:
        scale = 255.0 if unit else 1.0
        extra = 0.0 if out.dtype == torch.uint8 or not unit else 255.0 * HALF_ULP_AT_1[out.dtype]
        err = float(np.abs(got * scale - level).max())
        print(f"{what}: max |out - level64| = {err:.5f} levels (band {BAND + extra:.4f})")
        assert err <= BAND + extra, (what, err)
        if out.dtype == torch.float32 or (out.dtype != torch.uint8 and not unit):      # the output rule: an 8-bit level, cast (divided by 255 in float32)
            q = torch.round(out.to(torch.float32) * scale)
            assert torch.equal(out, ((q / 255.0) if unit else q).to(out.dtype)), what
        return err
    assert not unit
    err = float(np.abs(got - level).max()) / 255.0
    bound = TOL + HALF_ULP_AT_1[out.dtype] if out.dtype in (torch.bfloat16, torch.float16) else TOL
    print(f"{what}: max |out - level64| = {err:.3e} on [0, 1] (bound {bound:.3e})")
    assert err <= bound, (what, err)
    if copied.any():      # a pixel with a NaN member: the background rule's bits
        want = hn.to_output(level[copied], in_dtype, out.dtype, False)
        assert torch.equal(out[torch.from_numpy(copied)], want), what
    return err


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [PACKS, ODD], ids=["packs", "odd"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_four_rows_against_float64(dev, lib, dtype, shape, channels_last):
    x = images_of(dtype, shape, channels_last, dev)
    index = index_of(dtype, shape).reshape(-1)
    for row in hn.ROWS:
        level, copied = reference(dtype, row)
        out = raw(lib, x, row_tensor(row, dev), CL if channels_last else 0)
        assert out.dtype == dtype
        check_levels(as_pixels(out, channels_last), dtype, False, level[index], copied[index], (str(dtype), shape, channels_last, row))
    if dtype in (torch.float32, torch.float16, torch.bfloat16):
        assert reference(dtype, hn.ROWS[0])[1].sum() > 100      # (NaN members were among the pixels)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [PACKS, ODD], ids=["packs", "odd"])
@pytest.mark.parametrize("flags", [OUT_FLAG[torch.bfloat16], OUT_FLAG[torch.float16], UNIT, UNIT | OUT_FLAG[torch.bfloat16], UNIT | OUT_FLAG[torch.float16], CLASSIC],
                         ids=["bf16", "f16", "unit_f32", "unit_bf16", "unit_f16", "classic"])
def test_uint8_tiles_float_outputs(dev, lib, flags, shape, channels_last):
    x = images_of(torch.uint8, shape, channels_last, dev)
    index = index_of(torch.uint8, shape).reshape(-1)
    for row in hn.ROWS[:2]:
        level, copied = reference(torch.uint8, row)
        out = raw(lib, x, row_tensor(row, dev), flags | (CL if channels_last else 0))
        assert out.dtype == out_dtype_of(x, flags)
        check_levels(as_pixels(out, channels_last), torch.uint8, bool(flags & UNIT), level[index], copied[index], (flags, shape, channels_last, row))
        if flags & UNIT and flags != UNIT:      # (the 16-bit / 255: the float32 quotient rounded to the type)
            assert torch.equal(out, raw(lib, x, row_tensor(row, dev), UNIT | (CL if channels_last else 0)).to(out.dtype))
        if flags == CLASSIC:      # a no-op
            assert torch.equal(out, raw(lib, x, row_tensor(row, dev), CL if channels_last else 0))


@pytest.mark.parametrize("shape", [PACKS, ODD], ids=["packs", "odd"])
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=[str(d).split(".")[-1] for d in DTYPES[1:]])
def test_normalize_0_1_divides_the_level_output_by_255(dev, lib, dtype, shape):
    """A float tile's / 255 is the output rule's: the level rounded to the tile's type, divided by 255 in float32 (float64 tiles: in
    float64), rounded to the type again -- an exact relation to the call without the flag, no tolerance."""
    for channels_last in (False, True):
        x = images_of(dtype, shape, channels_last, dev)
        rows = row_tensor(hn.ROWS[1], dev)
        layout = CL if channels_last else 0
        level, unit = raw(lib, x, rows, layout).cpu(), raw(lib, x, rows, layout | UNIT).cpu()      # (divided on the CPU: the IEEE quotient)
        want = level / 255.0 if dtype == torch.float64 else (level.to(torch.float32) / 255.0).to(dtype)
        assert torch.equal(unit, want), (dtype, shape, channels_last)


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_pointers_one_element_off_give_the_aligned_bits(dev, lib, dtype):
    x = images_of(dtype, PACKS, False, dev)[:2].contiguous()
    rows = row_tensor(hn.ROWS[:2], dev)
    mask = (torch.rand(x.shape[0], *PACKS, device=dev) < 0.7).to(torch.uint8)
    want, want_masked = raw(lib, x, rows), raw(lib, x, rows, mask=mask)
    assert torch.equal(raw(lib, off_by_one(x), rows), want)
    out = off_by_one(torch.empty_like(want))
    assert torch.equal(raw(lib, x, rows, out=out), want)
    assert torch.equal(raw(lib, x, rows, mask=off_by_one(mask)), want_masked)
    assert torch.equal(raw(lib, off_by_one(x), rows, mask=mask), want_masked)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(raw(lib, off_by_one(nhwc), rows, CL).permute(0, 3, 1, 2), want)


# ------------------------------------------------------------------ rows
@pytest.mark.parametrize("shape", [PACKS, ODD], ids=["packs", "odd"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32], ids=["uint8", "bfloat16", "float32"])
def test_rows_per_tile_one_row_and_non_finite_rows(dev, lib, dtype, shape):
    x = images_of(dtype, shape, False, dev)[:3].contiguous()
    rows = row_tensor(hn.ROWS[:3], dev)
    out = raw(lib, x, rows)
    for t in range(3):      # tile t of the 3-tile call is the one-tile call with row t, bit for bit
        assert torch.equal(out[t:t + 1], raw(lib, x[t:t + 1].contiguous(), rows[t:t + 1].contiguous())), t
    assert torch.equal(raw(lib, x, rows[1:2].contiguous()), raw(lib, x, rows[1:2].repeat(3, 1)))
    background = raw(lib, x, row_tensor([float("nan")] * 5, dev))      # the background rule: uint8 tiles are the input's bytes
    if dtype == torch.uint8:
        assert torch.equal(background, x)
    else:
        assert torch.equal(as_pixels(background, False), hn.to_output(np.clip(np.nan_to_num(hn.input_levels(as_pixels(x, False)), nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0), dtype, dtype, False))
    for bad in (float("nan"), float("inf"), float("-inf")):
        for member in range(5):
            for t in range(3):
                spoiled = rows.clone()
                spoiled[t, member] = bad
                got = raw(lib, x, spoiled)
                others = [k for k in range(3) if k != t]
                assert torch.equal(got[t], background[t]) and torch.equal(got[others], out[others]), (bad, member, t)


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("shape", [PACKS, ODD], ids=["packs", "odd"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_masks(dev, lib, dtype, shape):
    x = images_of(dtype, shape, False, dev)[:3].contiguous()
    rows = row_tensor(hn.ROWS[:3], dev)
    plain = raw(lib, x, rows)
    background = raw(lib, x, row_tensor([float("nan")] * 5, dev))
    assert torch.equal(raw(lib, x, rows, mask=torch.ones(3, *shape, dtype=torch.uint8, device=dev)), plain)
    assert torch.equal(raw(lib, x, rows, mask=torch.zeros(3, *shape, dtype=torch.uint8, device=dev)), background)
    mask = (torch.rand(3, *shape, device=dev) < 0.6).to(torch.uint8) * 255      # (non-zero = in)
    got = raw(lib, x, rows, mask=mask)
    assert torch.equal(got, torch.where(mask.bool().unsqueeze(1), plain, background))
    if dtype == torch.uint8:
        assert torch.equal(got[~mask.bool().unsqueeze(1).expand_as(got)], x[~mask.bool().unsqueeze(1).expand_as(x)])      # the input's bytes
    # values under masked-out pixels do not matter: NaN / Inf / anything there, the masked-in pixels keep their bits
    junk = x.clone()
    out_px = ~mask.bool().unsqueeze(1).expand_as(x)
    junk[out_px] = torch.tensor(float("nan") if dtype != torch.uint8 else 7).to(dtype)
    assert torch.equal(raw(lib, junk, rows, mask=mask)[~out_px], got[~out_px])
    for flags in ((UNIT,) if dtype != torch.uint8 else (UNIT, OUT_FLAG[torch.bfloat16])):
        assert torch.equal(raw(lib, x, rows, flags, mask=mask), torch.where(mask.bool().unsqueeze(1), raw(lib, x, rows, flags), raw(lib, x, row_tensor([float("inf")] * 5, dev), flags)))


def test_luminosity_rule_is_the_explicit_tissue_mask(dev):
    x = images_of(torch.uint8, PACKS, False, dev)[:4].contiguous()
    rows = row_tensor(hn.ROWS, dev)
    explicit, counts = tissue_mask(x, 0.7)
    assert 0 < int(counts.sum()) < explicit.numel()
    want = adjust_hsv(x, rows, mask=explicit)
    assert torch.equal(adjust_hsv(x, rows, mask="luminosity", luminosity_threshold=0.7), want)
    assert torch.equal(HSVAugment(mask="luminosity", luminosity_threshold=0.7, normalize_to_0_1=False)(x, rows), want)
    assert torch.equal(HSVAugment(normalize_to_0_1=False)(x, rows, mask=explicit.unsqueeze(1)), want)
    assert not torch.equal(want, adjust_hsv(x, rows))


# ------------------------------------------------------------------ the module
def test_module_and_functional_form(dev, lib):
    x = images_of(torch.uint8, PACKS, False, dev)[:4].contiguous()
    rows = row_tensor(hn.ROWS, dev)
    want = raw(lib, x, rows)
    assert torch.equal(adjust_hsv(x, rows), want)
    with pytest.raises(ValueError, match="runs on a CUDA"):      # (the functional form follows its tensor: a CPU tensor has no GPU to follow)
        adjust_hsv(x.cpu(), rows)
    aug = HSVAugment(normalize_to_0_1=False)
    assert torch.equal(aug(x, rows), want)
    assert torch.equal(HSVAugment()(x, rows), raw(lib, x, rows, UNIT))      # normalize_to_0_1 defaults to True, as HEDAugment's
    assert torch.equal(adjust_hsv(x, rows, out_dtype=torch.bfloat16), raw(lib, x, rows, OUT_FLAG[torch.bfloat16]))
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(adjust_hsv(nhwc, rows, channel_axis=-1), want.permute(0, 2, 3, 1))
    # one row for the batch, in its three shapes
    one = raw(lib, x, rows[2:3].contiguous())
    assert torch.equal(adjust_hsv(x, rows[2]), one) and torch.equal(adjust_hsv(x, rows[2:3]), one) and torch.equal(aug(x, rows[2].cpu()), one)
    # CHW in, CHW out
    single = aug(x[1], rows[1])
    assert tuple(single.shape) == tuple(x[1].shape) and torch.equal(single, raw(lib, x[1:2].contiguous(), rows[1:2].contiguous())[0])
    assert torch.equal(adjust_hsv(x[1], rows[1:2]), single)
    # p = 0: every row is NaN, the input comes back exactly; p = 1 with zero magnitudes: the identity rows, the same
    assert torch.equal(HSVAugment(p=0.0, normalize_to_0_1=False)(x), x)
    assert torch.equal(HSVAugment(0.0, 0.0, 0.0, normalize_to_0_1=False)(x), x)
    # a draw: the rows sample_rows gives with the same seed, on the device when the generator is there
    for where in ("cpu", dev):
        gen = torch.Generator(device=where).manual_seed(5)
        drawn = HSVAugment(0.1, 0.3, 0.2, saturation_shift=0.05, value_shift=0.05, p=0.5, normalize_to_0_1=False, generator=gen)
        got = drawn(x)
        again = HSVAugment(0.1, 0.3, 0.2, saturation_shift=0.05, value_shift=0.05, p=0.5, normalize_to_0_1=False, generator=torch.Generator(device=where).manual_seed(5))
        rows_again = again.sample_rows(4, dev)
        assert torch.equal(got, raw(lib, x, rows_again.contiguous()))
        left = torch.isnan(rows_again).any(dim=1)
        assert torch.equal(got[left], x[left])


# ------------------------------------------------------------------ capture
def graph_nodes(dev) -> tuple[list[int], int, int]:
    """(node types, root nodes, edges) of the graph the current stream is capturing (hipStreamGetCaptureInfo_v2, hipGraphGetNodes)."""
    loaded = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]      # (the runtime torch loaded, not a second copy)
    hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipStreamGetCaptureInfo_v2.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetRootNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    status, ident, graph, deps, n_deps = ctypes.c_int(0), ctypes.c_ulonglong(0), vp(), vp(), sz(0)
    assert hip.hipStreamGetCaptureInfo_v2(_native.stream_ptr(dev), ctypes.byref(status), ctypes.byref(ident), ctypes.byref(graph), ctypes.byref(deps), ctypes.byref(n_deps)) == 0
    assert status.value == 1 and graph.value      # hipStreamCaptureStatusActive
    count = sz(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
    nodes = (vp * max(count.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(count)) == 0
    types = []
    for i in range(count.value):
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(nodes[i], ctypes.byref(kind)) == 0
        types.append(kind.value)
    roots, edges = sz(0), sz(0)
    assert hip.hipGraphGetRootNodes(graph, None, ctypes.byref(roots)) == 0 and hip.hipGraphGetEdges(graph, None, None, ctypes.byref(edges)) == 0
    return types, roots.value, edges.value


def test_a_captured_forward_replays_with_new_rows(dev):
    x = images_of(torch.uint8, PACKS, False, dev)[:4].contiguous()
    first, second = row_tensor(hn.ROWS, dev), row_tensor(hn.ROWS[::-1], dev)
    aug = HSVAugment(normalize_to_0_1=False)
    want_first, want_second = aug(x, first), aug(x, second)
    assert not torch.equal(want_first, want_second)
    buf = first.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream)
        aug(x, buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = aug(x, buf)
        types, roots, edges = graph_nodes(dev)
    assert types == [0], types      # ONE node, a kernel (hipGraphNodeTypeKernel = 0): no memset node (2), no copy (1)
    assert roots == 1 and edges == 0      # a single branch
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_first)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_second)
