"""The PRODUCT library's two forms of the Macenko transform pinned to each other bit for bit.

By default `libstainx_hip.so` runs the two-pass form (macenko_twopass.hpp) on big batches of mid-sized tiles and the four passes
(SX_MACENKO_CLASSIC) everywhere else; the two are meant to give the same bits.  test_twopass_gpu.py checks that on the diagnostic
build (-DSX_DIAG -DSX_STAMPS), which is not the code users load: the product has host code of its own (the demotion of unaligned
pointers and partial packs, the dense-record-only two-pass form, the size gates of sx_macenko_form, the refusal of the diagnostic
flags), and its kernels are compiled without the stage time stamps and environment knobs.  This module runs the product only,
through its C ABI (MacenkoHIP's router may send a flag-less call to the four passes after a hard batch, which would compare the
four passes with themselves), and holds its default form to its four-pass form bit for bit, where an oracle tolerance is blunt:
an off-by-one rank in a nearest-rank percentile, or the wrong key of a tie group, can stay inside 2.55e-2 on 512 x 512 tiles.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from stainx_amd import _native, synth
from tests.golden.cases import real_quadrants_512

pytestmark = pytest.mark.gpu

F32, U8, BF16, F16 = torch.float32, torch.uint8, torch.bfloat16, torch.float16
UNIT, NHWC, CLASSIC = _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC
OUT_BF16, OUT_F16 = _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16
SM = torch.tensor(synth.HE_REF, dtype=torch.float32)
TMC = torch.tensor([1.9705, 1.0308], dtype=torch.float32)
PARAM_KEYS = ("n_kept", "use_all", "vecs", "he", "max_c", "phi_lo", "phi_hi", "cov")
WHITE = (0, 15)      # the white tiles of the hard batch (_hard_batch)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """The library MacenkoHIP(dev) loads -- the product, unless the environment swaps it (test_the_product_library_is_loaded)."""
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev)._lib


@pytest.fixture(scope="module")
def ref(dev):
    return SM.to(dev), TMC.to(dev)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _tissue512() -> torch.Tensor:
    return synth.he_batch(64, 512, 512, seed0=6100)


def _tissue(n: int, h: int, w: int) -> torch.Tensor:
    """n uint8 tissue tiles of h x w: the 512 x 512 tiles themselves, or crops at their four corners (tile i from source i % 64)."""
    base = _tissue512()
    if (h, w) == (512, 512):
        assert n <= 64
        return base[:n].clone()
    corners = [(y, x) for y in (0, 512 - h) for x in (0, 512 - w)]
    assert n <= 64 * len(corners)
    return torch.stack([base[i % 64, :, corners[i // 64][0]:corners[i // 64][0] + h, corners[i // 64][1]:corners[i // 64][1] + w] for i in range(n)]).contiguous()


def _off_lattice(x: torch.Tensor, seed: int, tiles=None) -> torch.Tensor:
    """float32 tiles moved off the k / 255 lattice (seeded uniform noise of +-1e-4, clamped to [0, 1]): the float path, not the 8-bit codes."""
    g = torch.Generator().manual_seed(seed)
    y = x.clone()
    idx = range(x.shape[0]) if tiles is None else tiles
    for i in idx:
        y[i] = (x[i] + (torch.rand(x[i].shape, generator=g) * 2 - 1) * 1e-4).clamp_(0.0, 1.0)
    return y


def _is_grey(t: torch.Tensor) -> bool:
    return bool(torch.equal(t, (t * 255).round() / 255))


def _hard_batch() -> torch.Tensor:
    """(16,3,512,512) uint8: white tiles (fewer than 3 kept pixels in the prior's sample: the prior gives up and every slot takes
    the slow exact path) at 0 and 15, noise, few-colour and 90 %-background tiles among tissue."""
    x = _tissue(16, 512, 512)
    for i in WHITE:
        x[i] = 250
    x[3] = synth.noise_u8((3, 512, 512), seed=61)
    x[12] = synth.noise_u8((3, 512, 512), seed=62)
    x[6] = (x[6] // 64) * 64 + 20
    x[9] = (x[9] // 96) * 96 + 30
    x[10, :, : int(512 * 0.9), :] = 255
    return x


def _to(x_u8: torch.Tensor, dt: torch.dtype, flags: int = 0) -> torch.Tensor:
    x = synth.as_dtype(x_u8, dt)
    return x.permute(0, 2, 3, 1).contiguous() if flags & NHWC else x


# ------------------------------------------------------------------------------------------------ the raw C ABI
def _dims(x: torch.Tensor, flags: int) -> tuple[int, int, int]:
    return (x.shape[0], x.shape[1], x.shape[2]) if flags & NHWC else (x.shape[0], x.shape[2], x.shape[3])


def _out_dtype(dt: torch.dtype, flags: int) -> torch.dtype:
    if dt == U8 and flags & OUT_BF16:
        return BF16
    if dt == U8 and flags & OUT_F16:
        return F16
    return F32 if dt == U8 and flags & UNIT else dt


def _buffer(shape, dtype, dev, offset: int = 0, fill: int = 0) -> torch.Tensor:
    """A tensor of `shape` that starts `offset` elements into a flat buffer, every byte `fill`."""
    numel = int(np.prod(shape))
    flat = torch.empty(numel + offset, dtype=dtype, device=dev)
    flat.view(torch.uint8).fill_(fill)
    return flat[offset:offset + numel].view(shape)


def _unaligned_copy(x: torch.Tensor, offset: int) -> torch.Tensor:
    y = _buffer(x.shape, x.dtype, x.device, offset)
    y.copy_(x)
    return y


def _workspace(lib, x, flags, dev) -> torch.Tensor:
    n, h, w = _dims(x, flags)
    return torch.full((int(lib.sx_macenko_workspace_bytes_for(_native.DTYPE_CODES[x.dtype], n, h, w, flags)),), 0x3C, dtype=torch.uint8, device=dev)


def _call(lib, x, out, flags, ws, ref) -> None:
    n, h, w = _dims(x, flags)
    rc = lib.sx_macenko_transform(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, ref[0].data_ptr(), ref[1].data_ptr(),
                                  flags, ws.data_ptr(), ws.numel(), _native.stream_ptr(x.device))
    _native.check(rc, f"sx_macenko_transform(flags={flags:#x}, {tuple(x.shape)} {x.dtype})", lib)


def _params(lib, ws, n) -> dict[str, torch.Tensor]:
    raw = torch.empty((n, _native.MACENKO_PARAM_FLOATS), dtype=torch.float32, device=ws.device)
    _native.check(lib.sx_macenko_tile_params(ws.data_ptr(), n, raw.data_ptr(), _native.stream_ptr(ws.device)), "sx_macenko_tile_params", lib)
    raw = raw.cpu()
    return {"n_kept": raw[:, 0].long(), "use_all": raw[:, 1].long(), "vecs": raw[:, 2:8].reshape(-1, 3, 2), "phi_lo": raw[:, 8], "phi_hi": raw[:, 9],
            "he": raw[:, 10:16].reshape(-1, 3, 2), "max_c": raw[:, 16:18], "fell_back": raw[:, 18].long(), "n_candidates": raw[:, 19:23].long(),
            "cov": raw[:, 23:32].reshape(-1, 3, 3)}


def _telemetry(lib, ws) -> int:
    """The running count of selections that left the speculative path (tile 0's state; only ever added to)."""
    off = int(lib.sx_macenko_telemetry_offset())
    torch.cuda.synchronize()
    return int(ws[off:off + 4].view(torch.int32).item()) & 0xFFFFFFFF


def _assert_same_bytes(a: torch.Tensor, b: torch.Tensor, what) -> None:
    ab, bb = a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)
    if not torch.equal(ab, bb):
        bad = (ab != bb).nonzero().flatten()
        first = int(bad[0]) // a.element_size()
        raise AssertionError(f"{what}: {bad.numel()} bytes differ; first at element {first}: {a.reshape(-1)[first].item()!r} vs {b.reshape(-1)[first].item()!r}")


def _forms_agree(lib, ref, x, flags: int = 0, *, x_classic=None, out_offset: int = 0, what=""):
    """The default call (`flags`) and the four-pass call (`flags | CLASSIC`, on `x_classic` if given) on one workspace: the same
    output bytes and the same per-tile intermediates.  Every case takes the two-pass form by the library's own rule (form 1), so
    a change of its thresholds cannot quietly turn a case into a comparison of the four passes with themselves."""
    n, h, w = _dims(x, flags)
    dev = x.device
    assert lib.sx_macenko_form(_native.DTYPE_CODES[x.dtype], n, h, w, flags) == 1, (what, "no longer takes the two-pass form")
    ws = _workspace(lib, x, flags, dev)
    odt = _out_dtype(x.dtype, flags)
    out = _buffer(x.shape, odt, dev, out_offset, 0x5A)
    classic = _buffer(x.shape, odt, dev, 0, 0xA5)      # (other filler bytes: an element neither call writes cannot look equal)
    before = _telemetry(lib, ws)
    _call(lib, x, out, flags, ws, ref)
    p = _params(lib, ws, n)
    slow = (_telemetry(lib, ws) - before) & 0xFFFFFFFF
    _call(lib, x if x_classic is None else x_classic, classic, flags | CLASSIC, ws, ref)
    pc = _params(lib, ws, n)
    torch.cuda.synchronize()
    for k in PARAM_KEYS:
        assert torch.equal(p[k], pc[k]), (what, k, (p[k].double() - pc[k].double()).abs().max().item())
    _assert_same_bytes(out, classic, what)
    return SimpleNamespace(out=out, params=p, slow=slow)


def _report(what, r) -> None:
    slow = ((r.params["fell_back"] & 15) != 0).nonzero().flatten().tolist()
    print(f"{what}: {r.slow} selections left the speculative path; tiles {slow}")


# ------------------------------------------------------------------------------------------------ 1. the product is what runs
def test_the_product_library_is_loaded(lib, dev, ref):
    """Every diagnostic flag bit is refused (SX_ERR_BAD_ARG, no kernel runs): this is not libstainx_diag.so, whatever STAINX_DIAG
    or STAINX_HIP_LIB say."""
    x = _tissue(1, 64, 64).to(dev)
    bits = [1 << k for k in range(32) if _native.MACENKO_DIAG_BITS & (1 << k)]
    assert len(bits) == 6
    for bit in bits:
        ws = _workspace(lib, x, bit, dev)
        out = _buffer(x.shape, x.dtype, dev, 0, 0x5A)
        rc = lib.sx_macenko_transform(x.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[x.dtype], 1, 64, 64, ref[0].data_ptr(), ref[1].data_ptr(),
                                      bit, ws.data_ptr(), ws.numel(), _native.stream_ptr(dev))
        assert rc == _native.SX_ERR_BAD_ARG, (bit, rc)
        assert "diagnostic build" in _native.last_error(lib), (bit, _native.last_error(lib))
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all()), bit


def test_form_thresholds(lib):
    """The controls at the edges of the rule: one tile fewer, or a batch just under 4 M pixels, takes the four passes."""
    f32 = _native.DTYPE_CODES[F32]
    assert lib.sx_macenko_form(f32, 15, 512, 512, 0) == 0
    assert lib.sx_macenko_form(f32, 83, 224, 224, 0) == 0
    assert lib.sx_macenko_form(f32, 16, 512, 512, 0) == 1 and lib.sx_macenko_form(f32, 84, 224, 224, 0) == 1
    assert lib.sx_macenko_form(f32, 16, 512, 512, CLASSIC) == 0


# ------------------------------------------------------------------------------------------------ 3. where the product takes the two-pass form
F32_SHAPES = [(16, 512, 512), (64, 512, 512), (84, 224, 224), (114, 192, 192), (40, 320, 400)]


@pytest.mark.parametrize("grey", [True, False], ids=["grey", "off_lattice"])
@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_f32_default_equals_four_pass(lib, dev, ref, shape, grey):
    x = synth.as_dtype(_tissue(*shape), F32)
    if not grey:
        x = _off_lattice(x, seed=shape[0] * 1000 + shape[1])
        assert not any(_is_grey(t) for t in x)
    r = _forms_agree(lib, ref, x.to(dev), what=(shape, grey))
    _report(f"f32 {shape} {'grey' if grey else 'off-lattice'}", r)


def test_f32_one_off_lattice_tile_among_grey_levels(lib, dev, ref):
    x = _off_lattice(synth.as_dtype(_tissue(16, 512, 512), F32), seed=77, tiles=[8])
    assert [_is_grey(t) for t in x] == [i != 8 for i in range(16)]
    _forms_agree(lib, ref, x.to(dev), what="one off-lattice tile")


@pytest.mark.parametrize("shape", [(16, 512, 512), (32, 364, 364), (64, 512, 512)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", [U8, BF16, F16], ids=["u8", "bf16", "f16"])
def test_narrow_default_equals_four_pass(lib, dev, ref, dt, shape):
    r = _forms_agree(lib, ref, _to(_tissue(*shape), dt).to(dev), what=(dt, shape))
    _report(f"{dt} {shape}", r)


LAYOUTS = [(F32, UNIT), (F32, NHWC), (BF16, UNIT), (BF16, NHWC), (F16, UNIT), (F16, NHWC), (U8, UNIT), (U8, NHWC),
           (U8, OUT_BF16), (U8, OUT_BF16 | UNIT), (U8, OUT_F16), (U8, OUT_F16 | UNIT)]


@pytest.mark.parametrize("dt,flags", LAYOUTS, ids=[f"{str(d).split('.')[-1]}-{f:#x}" for d, f in LAYOUTS])
def test_unit_scale_layout_and_output_types(lib, dev, ref, dt, flags):
    x = _to(_tissue(16, 512, 512), dt, flags).to(dev)
    _forms_agree(lib, ref, x, flags, what=(dt, flags))


# ------------------------------------------------------------------------------------------------ 4. what the product sends back to the four passes
@pytest.mark.parametrize("dt", [U8, BF16, F16, F32], ids=["u8", "bf16", "f16", "f32"])
def test_tiles_of_partial_packs(lib, dev, ref, dt):
    """362 x 366 = 132 492 pixels, not a whole number of 16-pixel (uint8) or 8-pixel (2-byte) packs: form 1 by size, demoted to
    the four passes at call time.  float32 (4-pixel packs) really runs the two-pass form there."""
    assert (362 * 366) % 16 != 0 and (362 * 366) % 8 != 0 and (362 * 366) % 4 == 0
    _forms_agree(lib, ref, _to(_tissue(36, 362, 366), dt).to(dev), what=(dt, "partial packs"))


UNALIGNED_IN = [(F32, 1, (16, 512, 512)), (U8, 3, (16, 512, 512)), (F32, 1, (84, 224, 224)), (BF16, 1, (32, 364, 364))]


@pytest.mark.parametrize("dt,offset,shape", UNALIGNED_IN, ids=["f32+1", "u8+3", "f32+1-224", "bf16+1-364"])
def test_unaligned_input(lib, dev, ref, dt, offset, shape):
    """The four passes one pixel at a time (pointers that are not 16-byte aligned) give the packed passes' bits: the same work
    items per tile (224 x 224 and 364 x 364 are rounded to whole packs) and the same pixels in each lane's fp32 runs of moments."""
    x = _to(_tissue(*shape), dt).to(dev)
    xu = _unaligned_copy(x, offset)
    assert xu.data_ptr() % 16 != 0
    _forms_agree(lib, ref, xu, x_classic=x, what=(dt, "input", offset, shape))


@pytest.mark.parametrize("dt,flags,offset", [(F32, 0, 1), (U8, 0, 3), (U8, UNIT, 1), (U8, OUT_BF16, 1)], ids=["f32+1", "u8+3", "u8-unit+1", "u8-bf16+1"])
def test_unaligned_output(lib, dev, ref, dt, flags, offset):
    _forms_agree(lib, ref, _to(_tissue(16, 512, 512), dt).to(dev), flags, out_offset=offset, what=(dt, flags, "output", offset))


# ------------------------------------------------------------------------------------------------ 5. the slow exact path, reached by data
SLOW = [("f32", F32, 0, True), ("f32_off_lattice", F32, 0, False), ("u8", U8, 0, True), ("u8_unit", U8, UNIT, True), ("u8_bf16", U8, OUT_BF16, True),
        ("bf16", BF16, 0, True), ("f32_nhwc", F32, NHWC, True)]


@pytest.mark.parametrize("name,dt,flags,grey", SLOW, ids=[c[0] for c in SLOW])
def test_slow_exact_path_reached_by_data(lib, dev, ref, name, dt, flags, grey):
    """White tiles keep fewer than 3 pixels in the prior's sample: the prior gives up speculating and every slot of those tiles
    selects over the whole tile.  Its key scratch is the output plane for 4-byte outputs and recomputed keys for narrower ones;
    both must give the four passes' bits."""
    x = _to(_hard_batch(), dt, flags)
    if not grey:
        x = _off_lattice(x, seed=5)
    r = _forms_agree(lib, ref, x.to(dev), flags, what=name)
    _report(f"hard batch {name}", r)
    fell = r.params["fell_back"] & 15
    assert r.slow > 0, name
    for i in WHITE:
        assert int(fell[i]) != 0, (name, i, fell.tolist())


# ------------------------------------------------------------------------------------------------ 6. real tissue
@pytest.fixture(scope="module")
def real_images(golden):
    return torch.from_numpy(golden("g11_real_images.npz")["images_u8"])


@pytest.mark.parametrize("dt", [F32, U8], ids=["f32", "u8"])
def test_real_quadrants(lib, dev, ref, real_images, dt):
    quads = torch.stack([real_images[i, :, y:y + 512, x:x + 512] for i, y, x in real_quadrants_512()]).contiguous()
    r = _forms_agree(lib, ref, synth.as_dtype(quads, dt).to(dev), what=("quadrants", dt))
    _report(f"real quadrants {dt}", r)


def _example_batch(imgs: torch.Tensor) -> torch.Tensor:
    """64 float32 tiles as the reference's example pipeline makes them (ToDtype(float32, scale=True), then a resized crop with
    antialias): fixed crop boxes of assorted sizes and aspects from the six 1024 x 1024 images, each resized to 512 x 512."""
    rng = np.random.default_rng(2024)
    tiles = []
    for t in range(64):
        side, aspect = float(rng.uniform(280, 1024)), float(rng.uniform(0.75, 1.333))
        bh = int(min(1024, max(200, round(side * aspect ** 0.5))))
        bw = int(min(1024, max(200, round(side / aspect ** 0.5))))
        if (bh, bw) == (512, 512):
            bw += 8
        y, x = int(rng.integers(0, 1024 - bh + 1)), int(rng.integers(0, 1024 - bw + 1))
        crop = imgs[t % 6:t % 6 + 1, :, y:y + bh, x:x + bw].float() / 255.0
        tiles.append(F.interpolate(crop, size=(512, 512), mode="bilinear", antialias=True, align_corners=False))
    return torch.cat(tiles).clamp_(0.0, 1.0).contiguous()


def test_reference_example_float_pipeline(lib, dev, ref, real_images):
    from oracle import stain_oracle as so

    x = _example_batch(real_images)
    assert not any(_is_grey(t) for t in x)
    r = _forms_agree(lib, ref, x.to(dev), what="example pipeline")
    _report("example pipeline", r)
    subset = list(range(0, 64, 9))
    want, params = so.macenko_transform(x[subset].numpy(), SM.numpy(), TMC.numpy(), return_params=True)
    got = r.out.cpu()[subset].numpy()
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.55e-2      # 0-255 scale
    for k, i in enumerate(subset):
        np.testing.assert_allclose(r.params["he"][i].numpy(), params[k]["he"], rtol=0, atol=5e-5)
        np.testing.assert_allclose(r.params["max_c"][i].numpy(), params[k]["max_c"], rtol=1e-4, atol=0)


# ------------------------------------------------------------------------------------------------ 7. a captured default call
def test_captured_default_form_replays_on_new_data(lib, dev, ref):
    """A C caller may capture the default form (the Python router never does): one capture, no parallel branches; the replay on
    another batch in the same buffer gives the eager four-pass call's bits on that batch."""
    tiles = synth.as_dtype(_tissue(32, 512, 512), F32)
    a, b = tiles[:16].to(dev), _off_lattice(tiles[16:], seed=9, tiles=[5]).to(dev)
    assert lib.sx_macenko_form(_native.DTYPE_CODES[F32], 16, 512, 512, 0) == 1
    x = a.clone()
    ws = _workspace(lib, x, 0, dev)
    out = _buffer(x.shape, F32, dev, 0, 0x5A)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        _call(lib, x, out, 0, ws, ref)      # (eager once on the capture stream: code objects loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _call(lib, x, out, 0, ws, ref)
    x.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    eager = _buffer(x.shape, F32, dev, 0, 0xA5)
    _call(lib, b, eager, CLASSIC, _workspace(lib, b, CLASSIC, dev), ref)
    torch.cuda.synchronize()
    _assert_same_bytes(out, eager, "replayed default form vs eager four passes")


# ------------------------------------------------------------------------------------------------ 8. determinism, tile independence
@pytest.mark.parametrize("dt", [F32, U8], ids=["f32", "u8"])
def test_default_form_is_deterministic_and_tile_independent(lib, dev, ref, dt):
    x = _to(_tissue(16, 512, 512), dt).to(dev)
    assert lib.sx_macenko_form(_native.DTYPE_CODES[dt], 16, 512, 512, 0) == 1
    assert lib.sx_macenko_form(_native.DTYPE_CODES[dt], 1, 512, 512, 0) == 0
    ws = _workspace(lib, x, 0, dev)
    first, second = _buffer(x.shape, dt, dev, 0, 0x5A), _buffer(x.shape, dt, dev, 0, 0xA5)
    _call(lib, x, first, 0, ws, ref)
    _call(lib, x, second, 0, ws, ref)
    one = x[7:8].contiguous()
    alone = _buffer(one.shape, dt, dev, 0, 0xA5)
    _call(lib, one, alone, 0, _workspace(lib, one, 0, dev), ref)
    torch.cuda.synchronize()
    _assert_same_bytes(first, second, (dt, "two default calls"))
    _assert_same_bytes(alone, first[7:8], (dt, "one tile alone vs its slice of the batch"))
