"""One-word code records of the two-pass Macenko transform (stainx_amd/csrc/macenko_twopass.hpp: PriorRecord::coded,
write_records_codes, prefetch_candidates_codes) against the four passes of the same library, BIT FOR BIT.

The prior decides per tile, from its presample, whether a float32 tile of a coded call is 8-bit levels.  Such a tile's candidates
travel from pass A to the estimate stage as one word of three codes (the stage looks the optical densities up again); every
other tile keeps 16-byte records, and pass A attempts no lookup on it.  A level tile with a non-level element the presample missed
is found out by pass A, which sends all four slots of the tile to the whole-tile exact select.  Whatever happened, the output is
the four-pass form's (SX_MACENKO_CLASSIC: code this does not touch).

Which calls reach the new code.  A call is coded only when its batch holds at least 2^20 pixels in tiles of a multiple of 16
pixels (macenko.hip: coded_size), and the product library takes no SX_MACENKO_TWO_PASS (a diagnostic flag it refuses): it runs the
two-pass form by its own rule, float32 batches from 2^22 pixels in tiles from 192 x 192.  So every case runs
  * on the diagnostic library with the form forced, at the small shape the case was specified with (which pins the 16-byte path
    of a call without codes: 6 x 160 x 192, 4 x 130 x 132 and 4 x 256 x 256 are all below 2^20 pixels) AND at the smallest batch
    of such tiles that is coded;
  * on the product library at a batch its own rule sends to the two-pass form (sx_macenko_form == 1 is asserted), through a
    fresh backend per call (a backend that saw slow slots routes its next calls to the four passes).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from stainx_amd import _native, synth

pytestmark = pytest.mark.gpu

F32 = torch.float32
CLASSIC, TWO_PASS, NO_CODES = _native.MACENKO_CLASSIC, _native.MACENKO_TWO_PASS, _native.MACENKO_NO_CODES
SM = torch.tensor(synth.HE_REF, dtype=torch.float32)
TMC = torch.tensor([1.9705, 1.0308], dtype=torch.float32)
K_LDS_KEYS = 16384      # macenko.hip kLdsKeys
TOL_255 = 2.55e-2       # 0-255 scale: the oracle tolerance of tests/test_macenko_gpu.py, test_coded_gpu.py, test_product_forms_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=["product", "diag"])
def kind(request):
    return request.param


def _backend(kind, dev):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev, diag=(kind == "diag"))


def _coded_call(n: int, h: int, w: int, dt) -> bool:
    return dt == F32 and (h * w) % 16 == 0 and n * h * w >= 1 << 20      # macenko.hip: coded_call / coded_size


def _both(kind, dev, x, extra: int = 0):
    """(two-pass output, its tile parameters, four-pass output) of one backend; the two-pass form forced (diag) or asserted (product)."""
    be = _backend(kind, dev)
    n, _, h, w = x.shape
    flags = (TWO_PASS | extra) if kind == "diag" else 0
    assert be._lib.sx_macenko_form(_native.DTYPE_CODES[x.dtype], n, h, w, flags) == 1, (kind, tuple(x.shape), x.dtype, "does not take the two-pass form")
    two = be.transform(x, SM, TMC, _extra_flags=flags)
    p2 = be.tile_params(n)
    assert kind == "diag" or be._classic_left == 0
    classic = be.transform(x, SM, TMC, _extra_flags=CLASSIC)
    torch.cuda.synchronize()
    return two, p2, classic


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def _differing_tiles(a: torch.Tensor, b: torch.Tensor) -> list[int]:
    a8, b8 = a.cpu().view(torch.uint8), b.cpu().view(torch.uint8)
    return [t for t in range(a.shape[0]) if not torch.equal(a8[t], b8[t])]


@functools.lru_cache(maxsize=None)
def _levels(n: int, h: int, w: int, seed0: int) -> torch.Tensor:
    return synth.he_batch(n, h, w, seed0=seed0)      # uint8; shared between the tests, never written to (callers clone)


def _off_levels(x: torch.Tensor, seed: int) -> torch.Tensor:
    """float32 tiles moved off the k / 255 lattice by less than a grey level's spacing (3.9e-3): +-5e-4, clamped to [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    return (x + (torch.rand(x.shape, generator=g) - 0.5) * 1e-3).clamp_(0.0, 1.0)


def _batches(kind, h: int, w: int, stated_n: int | None):
    """Tile counts for tiles of h x w: diag -- the stated small batch (no codes) and the smallest coded batch; product -- the smallest batch
    the library's rule sends to the two-pass form (2^22 pixels; it is coded too where the tile allows)."""
    pixels = h * w
    if kind == "product":
        return [-(-(1 << 22) // pixels)] if pixels >= 36864 else []
    out = [stated_n] if stated_n else []
    if pixels % 16 == 0:
        out.append(max(-(-(1 << 20) // pixels), stated_n or 0))
    return sorted(set(out))


# ------------------------------------------------------------------------------------------------ 1. all-level tiles
def _all_level_cases():
    """(kind, n, h, w): the small batches on the diagnostic library, the coded batches of the same tiles, and the one shape of the three
    whose tiles the product library's rule sends to the two-pass form (tiles below 192 x 192 run in its four passes: no case)."""
    return [(kind, n, h, w) for (n0, h, w) in [(6, 160, 192), (4, 130, 132), (10, 332, 324)] for kind in ("product", "diag") for n in _batches(kind, h, w, n0)]


@pytest.mark.parametrize("case", _all_level_cases(), ids=lambda c: "-".join(map(str, c)))
def test_all_level_tiles(dev, case):
    """u8 / 255 tiles.  130 x 132 and 332 x 324: a partial last sweep of pass A and a pixel count that is no multiple of 1024 (130 x 132
    is no multiple of 16 either: never coded); 332 x 324 is the coded shape with those properties."""
    kind, n, h, w = case
    x = synth.as_dtype(_levels(n, h, w, 8100 + h), F32)
    two, p2, classic = _both(kind, dev, x.to(dev))
    assert _same(two, classic), (kind, n, h, w, _differing_tiles(two, classic))
    assert int((p2["fell_back"] & 15).max()) == 0, (kind, n, h, w, p2["fell_back"])
    assert int(p2["n_candidates"].min()) > 0, (kind, n, h, w)


def test_all_level_tiles_match_the_oracle(dev):
    from oracle import stain_oracle as so

    n, h, w = 35, 160, 192      # the smallest coded batch of the first shape
    assert _coded_call(n, h, w, F32)
    x = synth.as_dtype(_levels(n, h, w, 8100 + h), F32)
    two, p2, classic = _both("diag", dev, x.to(dev))
    assert _same(two, classic) and int((p2["fell_back"] & 15).max()) == 0
    want = so.macenko_transform(x.numpy(), SM.numpy(), TMC.numpy())
    assert np.abs(two.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max() <= TOL_255


# ------------------------------------------------------------------------------------------------ 2. mixed batch
def _mixed(n: int, h: int, w: int) -> torch.Tensor:
    x = synth.as_dtype(_levels(n, h, w, 8200), F32).clone()
    x[1::2] = _off_levels(x[0::2][: x[1::2].shape[0]], 82)      # odd tiles: the even tiles' pixels, off the lattice
    return x


def test_mixed_batch(kind, dev):
    """Even tiles are levels (4-byte records in a coded call), odd tiles the same tiles after a sub-LSB perturbation (16-byte records)."""
    shapes = [(n, 160, 192) for n in _batches(kind, 160, 192, 6)] + [(n, 384, 384) for n in _batches(kind, 384, 384, None)]
    assert shapes
    for n, h, w in shapes:
        x = _mixed(n, h, w).to(dev)
        two, p2, classic = _both(kind, dev, x)
        assert _same(two, classic), (kind, n, h, w, _differing_tiles(two, classic))
        assert int((p2["fell_back"][0::2] & 15).max()) == 0, (kind, n, h, w, p2["fell_back"])      # the level tiles did not fall back
        if kind == "diag":      # (the product library refuses the flag)
            plain, pp, _ = _both(kind, dev, x, extra=NO_CODES)
            assert _same(plain, classic), (kind, n, h, w, "no codes", _differing_tiles(plain, classic))


# ------------------------------------------------------------------------------------------------ 3. one non-level element
def _prior_sample_mask(h: int, w: int) -> np.ndarray:
    """True where prior_kernel looks (prior_fetch: unit u is one 16-pixel sector of cell u at a hashed offset; make_geometry's prior_units)."""
    n_sectors = h * w // 16
    units = min(max(n_sectors // 4, min(n_sectors, 64)), 1024)
    step = (n_sectors << 16) // units
    mask = np.zeros(h * w, dtype=bool)
    for u in range(units):
        start = (u * step) >> 16
        width = (((u + 1) * step) >> 16) - start
        sector = start + (((((u * 0x9E3779B1) & 0xFFFFFFFF) >> 16) * width) >> 16)
        mask[16 * sector:16 * sector + 16] = True
    return mask


@pytest.mark.parametrize("odd", ["half-level", "nan", "1.5"])
def test_level_tiles_with_a_single_non_level_element(kind, dev, odd):
    """Tiles 0 ... 3 of a batch of 256 x 256 level tiles get ONE odd element each, at different places: in tiles 0 and 2 inside the prior's
    presample (the prior says `not coded`: plain pass A, 16-byte records), in tiles 1 and 3 outside it (the prior says `coded`, a wave of
    pass A meets the element: all four slots of the tile take the whole-tile select).  Tile 1 is the tile that must report a fall-back --
    in a coded call, which 4 x 256 x 256 (2^18 pixels) is not: the batch is 16 tiles here (64 on the product library), the smallest coded one.
    No tile may differ from the four passes, whichever side of the sample its element fell on."""
    h = w = 256
    sampled = _prior_sample_mask(h, w)
    inside, outside = np.flatnonzero(sampled), np.flatnonzero(~sampled)
    places = [(0, int(inside[len(inside) // 3])), (1, int(outside[len(outside) // 2])), (2, int(inside[-1])), (1, int(outside[7]))]      # (channel, pixel) of tile t
    ran = 0
    for n in _batches(kind, h, w, 4):
        base = synth.as_dtype(_levels(n, h, w, 8300), F32)
        x = base.clone()
        for t, (c, p) in enumerate(places):
            k = int(round(float(base[t, c].view(-1)[p]) * 255.0))
            x[t, c].view(-1)[p] = {"half-level": (min(k, 254) + 0.5) / 255.0, "nan": float("nan"), "1.5": 1.5}[odd]
        two, p2, classic = _both(kind, dev, x.to(dev))
        fb = (p2["fell_back"] & 15).tolist()
        print(f"{kind} {odd} n={n}: fell_back of tiles 0-3 {fb[:4]}, the others {sorted(set(fb[4:]))}")
        assert _differing_tiles(two, classic) == [], (kind, odd, n, _differing_tiles(two, classic))
        if _coded_call(n, h, w, F32):
            assert fb[1] != 0 and fb[3] != 0, (kind, odd, n, fb[:4])      # the element the presample did not hit
            if odd != "nan":      # (a NaN inside the sample leaves the prior without a plane: that tile is slow for a reason of its own)
                assert fb[0] == 0 and fb[2] == 0, (kind, odd, n, fb[:4])
            assert max(fb[4:]) == 0
        ran += 1
    assert ran


# ------------------------------------------------------------------------------------------------ 4. more candidates than kLdsKeys
def _pure_stain_colour(stain: int, seed: int) -> torch.Tensor:
    """One uint8 colour of (almost) one pure stain: beyond every mixed pixel of a synthetic tile in angle."""
    rng = np.random.default_rng(seed)
    he = np.asarray(synth.HE_REF, dtype=np.float64)
    main = rng.uniform(0.9, 1.5) if stain == 0 else rng.uniform(0.7, 1.1)
    other = rng.uniform(0.0, 0.02)
    od = he @ (np.array([main, other]) if stain == 0 else np.array([other, main]))
    return torch.from_numpy(np.clip(np.round(240.0 * np.exp(-od)), 0, 255).astype(np.uint8))


def test_more_candidates_than_the_lds_key_array(kind, dev):
    """22 000 pixels (8.4 % of a 512 x 512 tile) of ONE pure-stain colour: the percentile is that colour and every one of them is a
    candidate -- more code records than kLdsKeys, selected on the speculative path with the keys beyond the array spilled to memory."""
    n = 16
    x8 = _levels(n, 512, 512, 8400).clone()
    for t, stain in ((12, 0), (13, 1)):
        x8[t].view(3, -1)[:, 5000:27000] = _pure_stain_colour(stain, 90 + t).view(3, 1)
    x = synth.as_dtype(x8, F32)
    assert _coded_call(n, 512, 512, F32)
    two, p2, classic = _both(kind, dev, x.to(dev))
    assert _same(two, classic), _differing_tiles(two, classic)
    spilled = [(t, s) for t in (12, 13) for s in range(4) if int(p2["n_candidates"][t, s]) > K_LDS_KEYS and not (int(p2["fell_back"][t]) >> s) & 1]
    print("slots with spilled keys on the speculative path:", spilled, p2["n_candidates"][[12, 13]].tolist())
    assert spilled


# ------------------------------------------------------------------------------------------------ 5. record overflow
def test_record_overflow_takes_the_slow_path(kind, dev):
    """Level tiles with a block of ONE pure-stain colour larger than the record array of a slot (512 x 512: 24576 records, macenko.hip
    dense_cap_for): every pixel of the block ties at the end of the slot's range and is a candidate.  The records beyond the array are
    dropped, the count says so, and the slot takes the whole-tile select; nothing is lost silently.  (A tile of one colour only, the
    construction of test_fused_gpu.py, gives the prior no plane: it never speculates and has no candidates at all.)"""
    n, cap = 16, 24576
    x8 = _levels(n, 512, 512, 8400).clone()
    built = {5: (0, 30000), 6: (1, 30000), 7: (0, 40000)}      # tile: (stain, pixels of the block)
    for t, (stain, count) in built.items():
        x8[t].view(3, -1)[:, 5000:5000 + count] = _pure_stain_colour(stain, 70 + t).view(3, 1)
    x = synth.as_dtype(x8, F32)
    assert _coded_call(n, 512, 512, F32)
    two, p2, classic = _both(kind, dev, x.to(dev))
    assert _same(two, classic), _differing_tiles(two, classic)
    over = [(t, s) for t in built for s in range(4) if int(p2["n_candidates"][t, s]) > cap]
    print(f"{kind}: candidates {p2['n_candidates'][list(built)].tolist()}, fell_back {[int(v) & 15 for v in p2['fell_back'][list(built)]]}; slots beyond the array {over}")
    assert over
    for t, s in over:
        assert (int(p2["fell_back"][t]) >> s) & 1, (t, s)
    plain = [t for t in range(n) if t not in built]
    assert int((p2["fell_back"][plain] & 15).max()) == 0


# ------------------------------------------------------------------------------------------------ 6. narrow pixels keep 16-byte records
@pytest.mark.parametrize("dt", [torch.uint8, torch.bfloat16], ids=["u8", "bf16"])
def test_uint8_and_bf16_batches(kind, dev, dt):
    if kind == "diag":
        shapes = [(6, 160, 192), (36, 160, 192)]
    else:
        shapes = [(16, 512, 512)]      # (narrow pixels: the product library's rule takes the two-pass form from 131072-pixel tiles)
    for n, h, w in shapes:
        x = synth.as_dtype(_levels(n, h, w, 8100 + h if h == 160 else 8400), dt)
        two, p2, classic = _both(kind, dev, x.to(dev))
        assert _same(two, classic), (kind, dt, n, _differing_tiles(two, classic))
        assert int((p2["fell_back"] & 15).max()) == 0, (kind, dt, n, p2["fell_back"])
