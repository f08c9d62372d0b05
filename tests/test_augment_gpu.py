"""Stain augmentation on the product library (include/stainx_hip.h: sx_macenko_augment; MacenkoHIP.augment; stainx_amd.MacenkoAugment).

* alpha = 1, beta = 0 with a fitted reference is the four-pass transform, bit for bit, on every path the transform has;
* own-basis and normalise-and-jitter modes against a numpy restatement built on the oracle's per-tile estimate, on the 24 real
  512 x 512 quadrants of the reference's example images;
* tiles are independent, alpha = beta = 0 is background, a captured call reads its factors at replay;
* argument errors at the Python level and at the C ABI; the module's sampling and its identity with StainNormalizerTransform.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import MacenkoAugment, StainNormalizerTransform, _native, synth

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC
TOL_255 = 2.55e-2      # float32 tiles on the 0-255 scale, as the transform's parity tests on these quadrants (tests/test_real_tissue.py)


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
    """The oracle's per-tile estimate of every quadrant (float32 and uint8 input): HE_source, maxC and the concentrations."""
    quads = real[3]
    out = {}
    for name, dt in (("f32", torch.float32), ("u8", torch.uint8)):
        x = synth.as_dtype(quads, dt).numpy()
        od = so.optical_density(so.to_unit_float(x))
        out[name] = [so.macenko_tile_params(od[i], signs="positive_sum") for i in range(len(x))]
    return out


def factors(n: int, seed: int, dev, s1: float = 0.25, s2: float = 0.2) -> tuple[torch.Tensor, torch.Tensor]:
    gen = torch.Generator().manual_seed(seed)
    alpha = 1.0 + s1 * (2.0 * torch.rand(n, 2, generator=gen) - 1.0)
    beta = s2 * (2.0 * torch.rand(n, 2, generator=gen) - 1.0)
    return alpha.to(dev), beta.to(dev)


def restated(x: np.ndarray, params: list[dict], alpha: np.ndarray, beta: np.ndarray, sm=None, tmc=None) -> np.ndarray:
    """C' = alpha C + beta (own basis, rebuilt with HE_source) or alpha (C tmc / maxC) + beta (rebuilt with SM); 240 exp(-OD'),
    clamped to [0, 255], cast as the transform casts."""
    n, _, h, w = x.shape
    out = np.empty((n, 3, h, w), dtype=np.float32)
    for i, p in enumerate(params):
        conc = p["conc"]
        if sm is None:
            basis = p["he"]
        else:
            basis = np.asarray(sm, dtype=np.float32)
            conc = conc * (np.asarray(tmc, dtype=np.float32) / p["max_c"])[:, None]
        conc = (alpha[i][:, None].astype(np.float32) * conc + beta[i][:, None].astype(np.float32)).astype(np.float32)
        od = (basis @ conc).astype(np.float32)
        out[i] = np.clip(so.IO * np.exp(-od), np.float32(0), np.float32(255)).reshape(3, h, w)
    return so.restore_dtype(out, x.dtype, in_0_255=True)


def assert_close_to(got: torch.Tensor, want: np.ndarray, name: str) -> None:
    diff = (got.cpu().double() - torch.from_numpy(want).double()).abs()
    if name == "u8":      # truncation to grey levels: a float difference of ~1e-3 moves a value across an integer now and then
        assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < 2e-3, (diff.max().item(), (diff > 0).float().mean().item())
    else:
        assert diff.max().item() <= TOL_255, diff.max().item()


# ------------------------------------------------------------------------------------------------ 1. identity = transform
def test_identity_is_the_four_pass_transform_bit_for_bit(dev, be, real):
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    u8_512 = synth.he_batch(64, 512, 512, seed0=2000)
    noisy = (u8_512[:16].float() / 255.0 + 1e-3 * torch.randn(16, 3, 512, 512, generator=torch.Generator().manual_seed(3))).clamp(0.0, 1.0)
    u8_224 = synth.he_batch(256, 224, 224, seed0=3000)
    cases = [
        ("f32 grey levels 64x512x512 (coded)", synth.as_dtype(u8_512, torch.float32), {}),
        ("f32 not grey levels", noisy, {}),
        ("u8", u8_512[:32], {}),
        ("u8 normalize_to_0_1", u8_512[:32], {"normalize_to_0_1": True}),
        ("u8 -> bf16", u8_512[:32], {"out_dtype": torch.bfloat16}),
        ("u8 -> f16 normalize_to_0_1", quads, {"out_dtype": torch.float16, "normalize_to_0_1": True}),
        ("bf16 256x224x224", synth.as_dtype(u8_224, torch.bfloat16), {}),
        ("f64", synth.as_dtype(u8_224[:4], torch.float64), {}),
        ("f32 NHWC", synth.as_dtype(quads[:8], torch.float32).permute(0, 2, 3, 1).contiguous(), {"channels_last": True}),
        ("u8 NHWC normalize_to_0_1", quads[8:16].permute(0, 2, 3, 1).contiguous(), {"channels_last": True, "normalize_to_0_1": True}),
    ]
    for name, x, kw in cases:
        x = x.to(dev)
        n = x.shape[0]
        ones, zeros = torch.ones(n, 2, device=dev), torch.zeros(n, 2, device=dev)
        want = be.transform(x, sm, tmc, _extra_flags=CLASSIC, **kw)
        got = be.augment(x, ones, zeros, sm, tmc, **kw)
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), name
        del x, got, want


# ------------------------------------------------------------------------------------------------ 2. / 3. against numpy
@pytest.mark.parametrize("name", ["f32", "u8"])
def test_own_basis_against_numpy(dev, be, real, oracle_params, name):
    quads = real[3]
    x = synth.as_dtype(quads, torch.float32 if name == "f32" else torch.uint8)
    alpha, beta = factors(len(x), 11, dev)
    got = be.augment(x.to(dev), alpha, beta)
    params = oracle_params[name]
    he = be.tile_params(len(x))["he"]
    for i, p in enumerate(params):
        np.testing.assert_allclose(he[i].numpy(), p["he"], rtol=0, atol=5e-5)
    assert_close_to(got, restated(x.numpy(), params, alpha.cpu().numpy(), beta.cpu().numpy()), name)


@pytest.mark.parametrize("name", ["f32", "u8"])
def test_normalise_and_jitter_against_numpy(dev, be, real, oracle_params, name):
    _, sm, tmc, quads = real
    x = synth.as_dtype(quads, torch.float32 if name == "f32" else torch.uint8)
    alpha, beta = factors(len(x), 12, dev)
    got = be.augment(x.to(dev), alpha, beta, sm.to(dev), tmc.to(dev))
    params = oracle_params[name]
    max_c = be.tile_params(len(x))["max_c"]
    for i, p in enumerate(params):
        np.testing.assert_allclose(max_c[i].numpy(), p["max_c"], rtol=1e-4, atol=0)
    assert_close_to(got, restated(x.numpy(), params, alpha.cpu().numpy(), beta.cpu().numpy(), sm.numpy(), tmc.numpy()), name)


# ------------------------------------------------------------------------------------------------ 4. / 5. tiles, background
def test_tiles_are_independent(dev, be, real):
    _, sm, tmc, _ = real
    x = synth.as_dtype(synth.he_batch(64, 256, 256, seed0=4000), torch.float32).to(dev)
    alpha, beta = factors(64, 13, dev)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5)).to(dev)
    for ref in ((), (sm.to(dev), tmc.to(dev))):
        out = be.augment(x, alpha, beta, *ref)
        out_p = be.augment(x[perm].contiguous(), alpha[perm].contiguous(), beta[perm].contiguous(), *ref)
        assert torch.equal(out_p, out[perm]), len(ref)


def test_no_stain_is_background(dev, be, real):
    _, sm, tmc, quads = real
    x = synth.as_dtype(quads[:6], torch.float32).to(dev)
    zeros = torch.zeros(6, 2, device=dev)
    for ref in ((), (sm.to(dev), tmc.to(dev))):
        assert (be.augment(x, zeros, zeros, *ref) - 240.0).abs().max().item() <= 1e-3
        assert (be.augment(x, zeros, zeros, *ref, normalize_to_0_1=True) - 240.0 / 255.0).abs().max().item() <= 1e-3 / 255.0


# ------------------------------------------------------------------------------------------------ 6. graph capture
def test_graph_replay_reads_new_images_and_factors(dev, be, real):
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)      # (on the device: a capture admits no host-to-device copy)
    first = synth.as_dtype(quads[:8], torch.float32).to(dev)
    second = synth.as_dtype(quads[8:16], torch.float32).to(dev)
    a1, b1 = factors(8, 21, dev)
    a2, b2 = factors(8, 22, dev)
    for ref in ((), (sm, tmc)):
        x, a, b = first.clone(), a1.clone(), b1.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                be.augment(x, a, b, *ref)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = be.augment(x, a, b, *ref)
        x.copy_(second)
        a.copy_(a2)
        b.copy_(b2)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, be.augment(second, a2, b2, *ref)), len(ref)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors(dev, be, real):
    _, sm, tmc, _ = real
    x = synth.as_dtype(synth.he_batch(2, 64, 64, seed0=5000), torch.float32).to(dev)
    ones, zeros = torch.ones(2, 2, device=dev), torch.zeros(2, 2, device=dev)
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        be.augment(x, torch.ones(2, 3, device=dev), zeros)
    with pytest.raises(ValueError, match="together"):
        be.augment(x, ones, zeros, sm.to(dev), None)
    assert be.augment(x[:0], ones[:0], zeros[:0]).shape == (0, 3, 64, 64)
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_macenko_workspace_bytes_for(f32, 2, 64, 64, CLASSIC))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty_like(x)
    smd, tmcd = sm.to(dev), tmc.to(dev)
    stream = _native.stream_ptr(dev)

    def call(alpha, beta, s, t, flags=0, nbytes=need):
        return lib.sx_macenko_augment(x.data_ptr(), out.data_ptr(), f32, 2, 64, 64, alpha, beta, s, t, flags, ws.data_ptr(), nbytes, stream)

    a, b = ones.data_ptr(), zeros.data_ptr()
    assert call(None, b, None, None) == _native.SX_ERR_BAD_ARG
    assert call(a, b, smd.data_ptr(), None) == _native.SX_ERR_BAD_ARG
    assert call(a, b, None, tmcd.data_ptr()) == _native.SX_ERR_BAD_ARG
    assert call(a, b, None, None, _native.MACENKO_SAMPLED) == _native.SX_ERR_BAD_ARG
    assert call(a, b, None, None, nbytes=need - 1) == _native.SX_ERR_WORKSPACE
    assert call(a, b, None, None, CLASSIC) == _native.SX_OK
    assert call(a, b, smd.data_ptr(), tmcd.data_ptr()) == _native.SX_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. the module
def test_module_sampling_and_identity(dev, real):
    imgs, _, _, quads = real
    x = synth.as_dtype(quads[:8], torch.float32).to(dev)
    outs = [MacenkoAugment(0.3, 0.25, generator=torch.Generator(device=dev).manual_seed(7))(x) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], MacenkoAugment(0.3, 0.25, generator=torch.Generator(device=dev).manual_seed(8))(x))
    m = MacenkoAugment(0.3, 0.25, generator=torch.Generator(device=dev).manual_seed(9))
    alpha, beta = m.sample_factors(100000, dev)
    assert alpha.shape == beta.shape == (100000, 2) and alpha.device == beta.device == x.device
    assert alpha.min().item() >= 0.7 - 1e-6 and alpha.max().item() <= 1.3 + 1e-6 and alpha.std().item() > 0.1
    assert beta.min().item() >= -0.25 - 1e-6 and beta.max().item() <= 0.25 + 1e-6 and beta.std().item() > 0.1
    a0, b0 = MacenkoAugment(0.0, 0.0).sample_factors(16, dev)
    assert torch.equal(a0, torch.ones(16, 2, device=dev)) and torch.equal(b0, torch.zeros(16, 2, device=dev))
    # a single CHW tile in, a CHW tile out; explicit factors
    one = m(x[0], torch.ones(1, 2, device=dev), torch.zeros(1, 2, device=dev))
    assert one.shape == x[0].shape
    # sigma = 0 with a reference: the normaliser module, bit for bit
    ref = imgs[0:1].to(dev)
    want = StainNormalizerTransform("macenko", reference=ref, device=dev, backend="torch_hip")(x)
    assert torch.equal(MacenkoAugment(0.0, 0.0, reference=ref)(x), want)
    u8 = quads[:8].to(dev)
    want8 = StainNormalizerTransform("macenko", reference=ref, device=dev, backend="torch_hip")(u8)
    assert torch.equal(MacenkoAugment(0.0, 0.0, reference=ref)(u8), want8)
    # a fitted Macenko as the normaliser
    from stainx_amd import Macenko

    fitted = Macenko(device=dev, backend="torch_hip").fit(ref)
    assert torch.equal(MacenkoAugment(0.0, 0.0, normalizer=fitted)(x), want)
