"""Stain separation on the product library (include/stainx_hip.h: sx_macenko_separate; MacenkoHIP.separate; Macenko.separate).

* the H image is sx_macenko_augment(alpha = (1, 0), beta = 0) and the E image alpha = (0, 1), bit for bit, in both modes, on every path
  the transform has (dtypes, coded and uncoded float32, NHWC, /255, uint8 -> bf16 / f16, partial packs, unaligned pointers);
* the concentration maps against a numpy restatement on the GPU's own per-tile estimate, and that estimate against the oracle;
* the per-tile outputs are what sx_macenko_tile_params reports; concentrations rebuild the transform's output;
* tiles are independent, background tiles follow the anchor, a captured call replays on new data.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stain_oracle as so
from stainx_amd import Macenko, StainSeparation, _native, synth

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC
TOL_255 = 2.55e-2      # float32 tiles on the 0-255 scale: the transform's parity bound on these quadrants (tests/test_real_tissue.py)
# The concentration fold C'_i = sum_j A_ij L_j + b_i rounds A (|A_ij| = ln2 s |pinv_ij| <~ 3) and b (|b_i| <~ 20) to float32 and
# evaluates three fmas: each term is off by half an ulp of its size (2^-24 relative), |A_ij L_j| <= 3 * 8 and |b_i| <= ~20, so the
# sum is off by a few ulps of ~32, about 1e-5 at worst.  The restatement's own float32 OD and product add ~1e-6.  Measured maximum on
# the 24 quadrants (MI355X): own basis 2.3e-6 (float32) / 1.9e-6 (uint8), normalised 3.0e-6 / 2.8e-6.
TOL_CONC = 3e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev)


@pytest.fixture(scope="module")
def real(golden):
    imgs = torch.from_numpy(golden("g11_real_images.npz")["images_u8"])
    g = golden("g11_real_tissue.npz")
    quads = torch.stack([imgs[i, :, y:y + 512, x:x + 512] for i in range(6) for y in (0, 512) for x in (0, 512)]).contiguous()
    return imgs, torch.from_numpy(g["stain_matrix"]), torch.from_numpy(g["target_max_conc"]), quads


@pytest.fixture(scope="module")
def oracle_params(real):
    quads = real[3]
    out = {}
    for name, dt in (("f32", torch.float32), ("u8", torch.uint8)):
        od = so.optical_density(so.to_unit_float(synth.as_dtype(quads, dt).numpy()))
        out[name] = [so.macenko_tile_params(od[i], signs="positive_sum") for i in range(len(od))]
    return out


def anchor(be, x, ref, **kw):
    """The H and E images by two augmentation calls: alpha = (1, 0) and (0, 1), beta = 0."""
    n = x.shape[0]
    zeros = torch.zeros(n, 2, device=x.device)
    e_h = torch.tensor([[1.0, 0.0]], device=x.device).expand(n, 2).contiguous()
    e_e = torch.tensor([[0.0, 1.0]], device=x.device).expand(n, 2).contiguous()
    return be.augment(x, e_h, zeros, *ref, **kw), be.augment(x, e_e, zeros, *ref, **kw)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def example_batch(imgs: torch.Tensor, n: int = 16) -> torch.Tensor:
    """float32 tiles off the k/255 lattice, as the reference's example pipeline makes them (a resized crop with antialias)."""
    rng = np.random.default_rng(2024)
    tiles = []
    for t in range(n):
        bh, bw = int(rng.integers(300, 1000)), int(rng.integers(300, 1000))
        y, x = int(rng.integers(0, 1024 - bh + 1)), int(rng.integers(0, 1024 - bw + 1))
        crop = imgs[t % 6:t % 6 + 1, :, y:y + bh, x:x + bw].float() / 255.0
        tiles.append(F.interpolate(crop, size=(512, 512), mode="bilinear", antialias=True, align_corners=False))
    return torch.cat(tiles).clamp_(0.0, 1.0).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the anchor: two augment calls
def test_images_are_the_augmentation_anchor_bit_for_bit(dev, be, real):
    imgs, sm, tmc, quads = real
    refs = ((), (sm.to(dev), tmc.to(dev)))
    u8_512 = synth.he_batch(64, 512, 512, seed0=2000)
    u8_224 = synth.he_batch(64, 224, 224, seed0=3000)
    cases = [
        ("f32 grey levels 64x512x512 (coded)", synth.as_dtype(u8_512, torch.float32), {}),
        ("f32 example pipeline (not grey levels)", example_batch(imgs), {}),
        ("u8", u8_512[:32], {}),
        ("u8 normalize_to_0_1", u8_512[:32], {"normalize_to_0_1": True}),
        ("f32 normalize_to_0_1", synth.as_dtype(quads, torch.float32), {"normalize_to_0_1": True}),
        ("u8 -> bf16", quads, {"out_dtype": torch.bfloat16}),
        ("u8 -> f16 normalize_to_0_1", quads, {"out_dtype": torch.float16, "normalize_to_0_1": True}),
        ("bf16 64x224x224", synth.as_dtype(u8_224, torch.bfloat16), {}),
        ("f16 64x224x224", synth.as_dtype(u8_224, torch.float16), {}),
        ("f64", synth.as_dtype(u8_224[:4], torch.float64), {}),
        ("f32 NHWC", synth.as_dtype(quads[:8], torch.float32).permute(0, 2, 3, 1).contiguous(), {"channels_last": True}),
        ("u8 NHWC normalize_to_0_1", quads[8:16].permute(0, 2, 3, 1).contiguous(), {"channels_last": True, "normalize_to_0_1": True}),
        ("bf16 NHWC", synth.as_dtype(u8_224[:8], torch.bfloat16).permute(0, 2, 3, 1).contiguous(), {"channels_last": True}),
        ("u8 321x199 (partial packs)", synth.he_batch(6, 321, 199, seed0=3500), {}),
        ("f32 321x199 (partial packs)", synth.as_dtype(synth.he_batch(6, 321, 199, seed0=3600), torch.float32), {}),
    ]
    for name, x, kw in cases:
        x = x.to(dev)
        for ref in refs:
            got = be.separate(x, *ref, concentrations=True, **kw)
            if ref:
                assert torch.isfinite(got["max_c"]).all() and (got["max_c"] != 0).all(), name      # (finite scales: the anchor is defined)
            want_h, want_e = anchor(be, x, ref, **kw)
            assert same_bits(got["stains"][0], want_h), (name, len(ref))
            assert same_bits(got["stains"][1], want_e), (name, len(ref))
        del x


def test_unaligned_pointers_at_the_c_abi(dev, be, real):
    """Input and output pointers one element off a 16-byte boundary: the scalar path, the anchor's bits all the same."""
    lib = _native.require()
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    stream = _native.stream_ptr(dev)
    for dt in (torch.float32, torch.uint8):
        x = synth.as_dtype(quads[:4, :, :256, :256], dt).contiguous().to(dev)
        n, numel = 4, x.numel()
        code = _native.DTYPE_CODES[dt]
        ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, n, 256, 256, CLASSIC)), dtype=torch.uint8, device=dev)
        src = torch.empty(numel + 1, dtype=dt, device=dev)
        src[1:].copy_(x.flatten())
        stains = torch.empty(2 * numel + 1, dtype=dt, device=dev)
        conc = torch.empty(n * 2 * 256 * 256 + 1, dtype=torch.float32, device=dev)
        aug = torch.empty(numel + 1, dtype=dt, device=dev)
        for ref in ((None, None), (sm.data_ptr(), tmc.data_ptr())):
            rc = lib.sx_macenko_separate(src[1:].data_ptr(), stains[1:].data_ptr(), conc[1:].data_ptr(), code, n, 256, 256, *ref, None, None, 0,
                                         ws.data_ptr(), ws.numel(), stream)
            assert rc == _native.SX_OK, _native.last_error()
            for k, alpha in enumerate(([1.0, 0.0], [0.0, 1.0])):
                a = torch.tensor([alpha], device=dev).expand(n, 2).contiguous()
                b = torch.zeros(n, 2, device=dev)
                rc = lib.sx_macenko_augment(src[1:].data_ptr(), aug[1:].data_ptr(), code, n, 256, 256, a.data_ptr(), b.data_ptr(), *ref, 0,
                                            ws.data_ptr(), ws.numel(), stream)
                assert rc == _native.SX_OK, _native.last_error()
                assert same_bits(stains[1 + k * numel:1 + (k + 1) * numel], aug[1:]), (dt, ref[0] is None, k)
            # the aligned call: the same concentrations
            aligned = be.separate(x, *((sm, tmc) if ref[0] else ()), stains=False, concentrations=True)["concentrations"]
            assert torch.equal(conc[1:].view(n, 2, 256, 256), aligned), dt
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. concentrations
def restated_conc(x: np.ndarray, he: np.ndarray, max_c: np.ndarray | None, tmc: np.ndarray | None) -> np.ndarray:
    """pinv(HE) @ optical_density(x) in float32 with the GPU's own HE_source, scaled by tmc / maxC in normalised mode."""
    od = so.optical_density(so.to_unit_float(x)).astype(np.float32)
    n, _, h, w = od.shape
    out = np.empty((n, 2, h, w), dtype=np.float32)
    for i in range(n):
        pinv = np.linalg.pinv(he[i].astype(np.float64)).astype(np.float32)
        c = pinv @ od[i].reshape(3, -1)
        if tmc is not None:
            c = c * (tmc.astype(np.float32) / max_c[i].astype(np.float32))[:, None]
        out[i] = c.reshape(2, h, w)
    return out


@pytest.mark.parametrize("name", ["f32", "u8"])
@pytest.mark.parametrize("normalised", [False, True])
def test_concentrations_against_numpy(dev, be, real, oracle_params, name, normalised):
    _, sm, tmc, quads = real
    x = synth.as_dtype(quads, torch.float32 if name == "f32" else torch.uint8)
    ref = (sm.to(dev), tmc.to(dev)) if normalised else ()
    got = be.separate(x.to(dev), *ref, stains=False, concentrations=True, max_conc=True)
    he, max_c = got["he"].cpu().numpy(), got["max_c"].cpu().numpy()
    for i, p in enumerate(oracle_params[name]):
        np.testing.assert_allclose(he[i], p["he"], rtol=0, atol=5e-5)
        np.testing.assert_allclose(max_c[i], p["max_c"], rtol=1e-4, atol=0)
    want = restated_conc(x.numpy(), he, max_c, tmc.numpy() if normalised else None)
    err = float(np.abs(got["concentrations"].cpu().numpy() - want).max())
    print(f"separate concentrations {name} normalised={normalised}: max |C' - numpy| = {err:.3e}")
    assert err <= TOL_CONC, err


# ------------------------------------------------------------------------------------------------ 3. per-tile outputs = tile_params
def test_tile_outputs_are_tile_params(dev, be, real, oracle_params):
    _, sm, tmc, quads = real
    x = synth.as_dtype(quads, torch.float32).to(dev)
    for ref, max_conc in (((), False), ((), True), ((sm.to(dev), tmc.to(dev)), False)):
        got = be.separate(x, *ref, max_conc=max_conc)
        tp = be.tile_params(len(x))
        assert torch.equal(got["he"].cpu(), tp["he"]), (len(ref), max_conc)
        if ref or max_conc:
            assert torch.equal(got["max_c"].cpu(), tp["max_c"]), (len(ref), max_conc)
            for i, p in enumerate(oracle_params["f32"]):
                np.testing.assert_allclose(got["max_c"][i].cpu().numpy(), p["max_c"], rtol=1e-4, atol=0)
        else:
            assert got["max_c"] is None


# ------------------------------------------------------------------------------------------------ 4. consistency
def test_concentrations_rebuild_the_transform(dev, be, real, oracle_params):
    _, sm, tmc, quads = real
    x = synth.as_dtype(quads, torch.float32).to(dev)
    smd, tmcd = sm.to(dev), tmc.to(dev)
    got = be.separate(x, smd, tmcd, concentrations=True)
    n, _, h, w = x.shape
    od = torch.einsum("cs,nshw->nchw", smd, got["concentrations"])
    rebuilt = (240.0 * torch.exp(-od)).clamp(0.0, 255.0)
    want = be.transform(x, smd, tmcd, _extra_flags=CLASSIC)
    assert (rebuilt - want).abs().max().item() <= TOL_255
    # the images against the oracle's estimate: torchstain's H and E with Io = 240
    smn, tmcn = sm.numpy().astype(np.float32), tmc.numpy().astype(np.float32)
    for i, p in enumerate(oracle_params["f32"]):
        c = p["conc"] * (tmcn / p["max_c"])[:, None]
        for s, img in enumerate((got["stains"][0][i], got["stains"][1][i])):
            ref_img = np.clip(so.IO * np.exp(-np.outer(smn[:, s], c[s])), 0, 255).reshape(3, h, w)
            assert np.abs(img.cpu().numpy() - ref_img).max() <= TOL_255, (i, s)


# ------------------------------------------------------------------------------------------------ 5. robustness
def test_tiles_are_independent(dev, be, real):
    _, sm, tmc, _ = real
    x = synth.as_dtype(synth.he_batch(32, 256, 256, seed0=4000), torch.float32).to(dev)
    for ref in ((), (sm.to(dev), tmc.to(dev))):
        batch = be.separate(x, *ref, concentrations=True)
        for i in (0, 17, 31):
            one = be.separate(x[i:i + 1].contiguous(), *ref, concentrations=True)
            assert torch.equal(one["stains"][:, 0], batch["stains"][:, i]), (i, len(ref))
            assert torch.equal(one["concentrations"][0], batch["concentrations"][i]), (i, len(ref))
            assert torch.equal(one["he"][0], batch["he"][i]), (i, len(ref))


def test_background_and_constant_tiles(dev, be, real):
    """An all-white tile (fewer than 3 kept pixels: the transform's fallback to every pixel) and constant tiles, next to tissue.
    Result: every such tile here has finite, non-zero maxC, so its images are the anchor's bits; a stain whose own scale were
    infinite would give the transform's arithmetic (non-finite values, clamped) for that stain only -- the other stain's image
    is checked against its own rebuild from the concentrations."""
    _, sm, tmc, quads = real
    tissue = synth.as_dtype(quads[:2], torch.float32)
    white = torch.ones(1, 3, 512, 512)
    pink = torch.tensor([0.85, 0.55, 0.75]).view(1, 3, 1, 1).expand(1, 3, 512, 512)
    grey = torch.full((1, 3, 512, 512), 0.5)
    x = torch.cat([tissue, white, pink, grey]).contiguous().to(dev)
    smd, tmcd = sm.to(dev), tmc.to(dev)
    for ref in ((), (smd, tmcd)):
        got = be.separate(x, *ref, concentrations=True, max_conc=True)
        assert torch.isfinite(got["he"]).all()
        max_c = got["max_c"].cpu()
        want_h, want_e = anchor(be, x, ref)
        basis = smd if ref else None
        for i in range(x.shape[0]):
            finite = bool(torch.isfinite(max_c[i]).all() and (max_c[i] != 0).all())
            if finite or not ref:
                assert torch.equal(got["stains"][0][i], want_h[i]) and torch.equal(got["stains"][1][i], want_e[i]), i
            for s in range(2):
                if ref and not (torch.isfinite(max_c[i, s]) and max_c[i, s] != 0):
                    continue
                m = (basis if basis is not None else got["he"][i])[:, s].view(3, 1, 1)
                rebuilt = (240.0 * torch.exp(-m * got["concentrations"][i, s])).clamp(0.0, 255.0)
                assert (rebuilt - got["stains"][s][i]).abs().max().item() <= TOL_255, (i, s)


def test_graph_replay_reads_new_images(dev, be, real):
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    first = synth.as_dtype(quads[:8], torch.float32).to(dev)
    second = synth.as_dtype(quads[8:16], torch.float32).to(dev)
    for ref in ((), (sm, tmc)):
        x = first.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                be.separate(x, *ref, concentrations=True, max_conc=True)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = be.separate(x, *ref, concentrations=True, max_conc=True)
        x.copy_(second)
        g.replay()
        torch.cuda.synchronize()
        want = be.separate(second, *ref, concentrations=True, max_conc=True)
        for k in ("stains", "concentrations", "he", "max_c"):
            assert torch.equal(out[k], want[k]), (k, len(ref))


# ------------------------------------------------------------------------------------------------ 6. errors at the C ABI, the public method
def test_c_abi_errors_and_success(dev, real):
    _, sm, tmc, _ = real
    lib = _native.require()
    x = synth.as_dtype(synth.he_batch(2, 64, 64, seed0=5000), torch.float32).to(dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_macenko_workspace_bytes_for(f32, 2, 64, 64, CLASSIC))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    stains = torch.empty(2, *x.shape, device=dev)
    conc = torch.empty(2, 2, 64, 64, device=dev)
    smd, tmcd = sm.to(dev), tmc.to(dev)

    def call(st=stains.data_ptr(), c=conc.data_ptr(), s=None, t=None, flags=0, nbytes=need):
        return lib.sx_macenko_separate(x.data_ptr(), st, c, f32, 2, 64, 64, s, t, None, None, flags, ws.data_ptr(), nbytes, _native.stream_ptr(dev))

    assert call(st=None, c=None) == _native.SX_ERR_BAD_ARG
    assert call(s=smd.data_ptr()) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_SAMPLED) == _native.SX_ERR_BAD_ARG
    assert call(nbytes=need - 1) == _native.SX_ERR_WORKSPACE
    assert call(flags=CLASSIC) == _native.SX_OK
    assert call(st=None, s=smd.data_ptr(), t=tmcd.data_ptr()) == _native.SX_OK
    torch.cuda.synchronize()


def test_public_method(dev, real):
    imgs, sm, tmc, quads = real
    x = quads[:4].to(dev)
    norm = Macenko(device=dev, backend="torch_hip")
    own = norm.separate(x, concentrations=True)
    assert isinstance(own, StainSeparation) and own.max_concentrations is None
    assert own.hematoxylin.shape == x.shape and own.hematoxylin.dtype == torch.uint8 and own.stain_matrices.shape == (4, 3, 2)
    assert own.concentrations.shape == (4, 2, 512, 512)
    norm.fit(imgs[0:1].to(dev))
    fitted = norm.separate(x)
    assert fitted.concentrations is None and fitted.max_concentrations.shape == (4, 2)
    want_h, want_e = anchor(norm._get_backend_impl(), x, (norm._stain_matrix.to(dev), norm._target_max_conc.to(dev)))
    assert torch.equal(fitted.hematoxylin, want_h) and torch.equal(fitted.eosin, want_e)
    assert torch.equal(norm.separate(x, own_basis=True).hematoxylin, own.hematoxylin)
    unit = Macenko(device=dev, backend="torch_hip", normalize_to_0_1=True, precision="fast").separate(x, stains=True)
    assert unit.hematoxylin.dtype == torch.float32 and unit.hematoxylin.max().item() <= 1.0
    half = Macenko(device=dev, backend="torch_hip", output_dtype=torch.bfloat16).separate(x)
    assert half.eosin.dtype == torch.bfloat16
