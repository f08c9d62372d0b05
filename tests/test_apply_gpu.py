"""Slide-level Macenko on the product library (include/stainx_hip.h: sx_macenko_estimate, sx_macenko_apply; MacenkoHIP.estimate / .apply;
Macenko.estimate / .apply).

* the anchor, bit for bit: a tile's own estimate fed back gives sx_macenko_transform(CLASSIC) (and the default form), with factors
  sx_macenko_augment in both modes; n_sources = 1 is n_sources = N with the row repeated; the estimate's outputs are what
  sx_macenko_tile_params reports -- on every path the transform has (dtypes, coded and uncoded float32, NHWC, /255, uint8 -> bf16 / f16,
  partial packs, unaligned pointers);
* against the reference's arithmetic with a source the GPU did not estimate (the numpy oracle's pooled fit, its per-tile estimates);
* degenerate tiles and sources stay defined; a captured call replays on new images, source and factors; the public methods.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stain_oracle as so
from stainx_amd import Macenko, StainEstimate, _native, synth

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC
TOL_255 = 2.55e-2      # float32 tiles on the 0-255 scale: the project's parity bound for this fold (tests/test_macenko_gpu.py, test_real_tissue.py)
HALF_BOUND = {torch.bfloat16: 1.0, torch.float16: 0.125}      # bf16 / f16 outputs: tests/test_macenko_gpu.py's bounds (one step of the type at 128-255 ...
HALF_SHARE = 2e-3                                              # ... on fewer than 0.2 % of the elements)
LOOSE_SHARE = 0.12     # uint8: at most this share of a quadrant may fall under the "within one level" half of the rule


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


def factors(n: int, dev, seed: int = 77):
    """A seeded draw: alpha in [0.7, 1.3], beta in [-0.2, 0.2], (H, E) per tile."""
    gen = torch.Generator().manual_seed(seed)
    alpha = 0.7 + 0.6 * torch.rand(n, 2, generator=gen)
    beta = -0.2 + 0.4 * torch.rand(n, 2, generator=gen)
    return alpha.to(dev), beta.to(dev)


# ------------------------------------------------------------------------------------------------ 1. the anchors, bit for bit
def anchor_cases(real):
    imgs, _, _, quads = real
    u8_512 = synth.he_batch(64, 512, 512, seed0=2000)
    u8_224 = synth.he_batch(64, 224, 224, seed0=3000)
    return [
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


def test_own_estimate_fed_back_is_the_transform_and_the_augmentation_bit_for_bit(dev, be, real):
    _, sm, tmc, _ = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    for name, x, kw in anchor_cases(real):
        x = x.to(dev)
        n = x.shape[0]
        nhwc = {"channels_last": True} if kw.get("channels_last") else {}
        # anchor 4: the estimate's outputs are sx_macenko_tile_params after a CLASSIC transform of the same batch
        want = be.transform(x, sm, tmc, _extra_flags=CLASSIC, **kw)
        tp = be.tile_params(n)
        est = be.estimate(x, **nhwc)
        he, max_c = est["he"], est["max_c"]
        assert same_bits(he.cpu(), tp["he"].contiguous()) and same_bits(max_c.cpu(), tp["max_c"].contiguous()), name
        assert torch.equal(est["tissue"].cpu().long(), tp["n_kept"]), name
        assert torch.isfinite(max_c).all() and (max_c != 0).all(), name      # (finite scales: the anchor is defined on EVERY tile)
        # anchor 1: no factors, the reference -> the transform, four-pass form and default form
        got = be.apply(x, he, max_c, sm, tmc, **kw)
        assert same_bits(got, want), name
        assert same_bits(got, be.transform(x, sm, tmc, **kw)), name
        # anchor 2: with factors -> the augmentation, normalise-and-jitter and own basis (no maxC given there)
        alpha, beta = factors(n, dev)
        assert same_bits(be.apply(x, he, max_c, sm, tmc, alpha=alpha, beta=beta, **kw), be.augment(x, alpha, beta, sm, tmc, **kw)), name
        assert same_bits(be.apply(x, he, None, alpha=alpha, beta=beta, **kw), be.augment(x, alpha, beta, **kw)), name
        # anchor 3: one source row for the batch = that row repeated; a tile's output does not depend on its batch
        j = n // 2
        one = be.apply(x, he[j:j + 1], max_c[j:j + 1], sm, tmc, alpha=alpha, beta=beta, **kw)
        rep = be.apply(x, he[j:j + 1].expand(n, 3, 2).contiguous(), max_c[j:j + 1].expand(n, 2).contiguous(), sm, tmc, alpha=alpha, beta=beta, **kw)
        assert same_bits(one, rep), name
        assert same_bits(be.apply(x, he[j], max_c[j], sm, tmc, **kw), be.apply(x, he[j:j + 1].expand(n, 3, 2).contiguous(), max_c[j:j + 1].expand(n, 2).contiguous(), sm, tmc, **kw)), name
        alone = be.apply(x[j:j + 1].contiguous(), he[j:j + 1], max_c[j:j + 1], sm, tmc, alpha=alpha[j:j + 1], beta=beta[j:j + 1], **kw)
        assert same_bits(alone[0], one[j]) and same_bits(be.apply(x[j:j + 1].contiguous(), he[j:j + 1], max_c[j:j + 1], sm, tmc, **kw)[0], got[j]), name
        del x, want, got, one, rep, alone


def test_unaligned_pointers_at_the_c_abi(dev, be, real):
    """Input and output pointers one element off a 16-byte boundary: the scalar path, the anchors' bits all the same."""
    lib = _native.require()
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    stream = _native.stream_ptr(dev)
    for dt in (torch.float32, torch.uint8, torch.bfloat16):
        x = synth.as_dtype(quads[:4, :, :256, :256], dt).contiguous().to(dev)
        n, numel = 4, x.numel()
        code = _native.DTYPE_CODES[dt]
        ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, n, 256, 256, CLASSIC)), dtype=torch.uint8, device=dev)
        src = torch.empty(numel + 1, dtype=dt, device=dev)
        src[1:].copy_(x.flatten())
        out, want = torch.empty(numel + 1, dtype=dt, device=dev), torch.empty(numel + 1, dtype=dt, device=dev)
        he, max_c, tissue = torch.empty(n, 3, 2, device=dev), torch.empty(n, 2, device=dev), torch.empty(n, device=dev)
        rc = lib.sx_macenko_estimate(src[1:].data_ptr(), code, n, 256, 256, he.data_ptr(), max_c.data_ptr(), tissue.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
        assert rc == _native.SX_OK, _native.last_error()
        assert torch.isfinite(max_c).all() and (max_c != 0).all(), dt
        alpha, beta = factors(n, dev)
        rc = lib.sx_macenko_transform(src[1:].data_ptr(), want[1:].data_ptr(), code, n, 256, 256, sm.data_ptr(), tmc.data_ptr(), CLASSIC, ws.data_ptr(), ws.numel(), stream)
        assert rc == _native.SX_OK, _native.last_error()
        raw = torch.empty(n, _native.MACENKO_PARAM_FLOATS, device=dev)
        assert lib.sx_macenko_tile_params(ws.data_ptr(), n, raw.data_ptr(), stream) == _native.SX_OK
        assert same_bits(he.view(n, 6), raw[:, 10:16].contiguous()) and same_bits(max_c, raw[:, 16:18].contiguous()) and same_bits(tissue, raw[:, 0].contiguous()), dt
        rc = lib.sx_macenko_apply(src[1:].data_ptr(), out[1:].data_ptr(), code, n, 256, 256, he.data_ptr(), max_c.data_ptr(), n, None, None, sm.data_ptr(), tmc.data_ptr(), 0, stream)
        assert rc == _native.SX_OK, _native.last_error()
        assert same_bits(out[1:], want[1:]), dt
        assert same_bits(out[1:].view_as(x), be.apply(x, he, max_c, sm, tmc)), dt      # (the aligned call: the same pixels)
        for ref in ((None, None), (sm.data_ptr(), tmc.data_ptr())):
            rc = lib.sx_macenko_augment(src[1:].data_ptr(), want[1:].data_ptr(), code, n, 256, 256, alpha.data_ptr(), beta.data_ptr(), *ref, 0, ws.data_ptr(), ws.numel(), stream)
            assert rc == _native.SX_OK, _native.last_error()
            rc = lib.sx_macenko_apply(src[1:].data_ptr(), out[1:].data_ptr(), code, n, 256, 256, he.data_ptr(), max_c.data_ptr() if ref[0] else None, n,
                                      alpha.data_ptr(), beta.data_ptr(), *ref, 0, stream)
            assert rc == _native.SX_OK, _native.last_error()
            assert same_bits(out[1:], want[1:]), (dt, ref[0] is None)
        # only the output off alignment, and only the input
        rc = lib.sx_macenko_apply(x.data_ptr(), out[1:].data_ptr(), code, n, 256, 256, he.data_ptr(), max_c.data_ptr(), n, None, None, sm.data_ptr(), tmc.data_ptr(), 0, stream)
        assert rc == _native.SX_OK and same_bits(out[1:].view_as(x), be.apply(x, he, max_c, sm, tmc)), dt
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the reference's arithmetic, a source the GPU did not estimate
def restated(x: np.ndarray, he: np.ndarray, max_c: np.ndarray, sm: np.ndarray, tmc: np.ndarray) -> np.ndarray:
    """The tail of the oracle's transform (oracle/stain_oracle.py:161-165) with a GIVEN (HE, maxC), one row for the batch or one per tile:
    float32 values on the 0-255 scale, before the cast to the image type."""
    sm, tmc = sm.astype(np.float32), tmc.astype(np.float32).reshape(-1)
    od_all = so.optical_density(so.to_unit_float(x))
    n, _, h, w = od_all.shape
    out = np.empty((n, 3, h, w), dtype=np.float32)
    for i in range(n):
        k = i if he.shape[0] == n else 0
        conc = so.concentrations(he[k], od_all[i].reshape(3, -1))
        scaled = conc * (tmc / max_c[k].astype(np.float32))[:, None]
        od_new = (sm @ scaled).astype(np.float32)
        out[i] = np.clip(so.IO * np.exp(-od_new), np.float32(0), np.float32(255)).reshape(3, h, w)
    return out


@pytest.fixture(scope="module")
def oracle_sources(real):
    """Sources by numpy alone: the pooled fit over the 24 quadrants and the per-tile estimates (float32 and uint8 quadrants hold the same
    unit values, so one set serves both)."""
    quads = real[3]
    xf = synth.as_dtype(quads, torch.float32).numpy()
    assert np.array_equal(so.to_unit_float(xf), so.to_unit_float(quads.numpy()))
    he, max_c = so.macenko_fit(xf, signs="positive_sum")
    od = so.optical_density(so.to_unit_float(xf))
    tiles = [so.macenko_tile_params(od[i], signs="positive_sum") for i in range(len(od))]
    per_tile = (np.stack([p["he"] for p in tiles]).astype(np.float32), np.stack([p["max_c"] for p in tiles]).astype(np.float32))
    for arr in (he, max_c, *per_tile):
        assert np.isfinite(arr).all()
    assert (max_c != 0).all() and (per_tile[1] != 0).all()
    return {"pooled": (he.astype(np.float32).reshape(1, 3, 2), max_c.astype(np.float32).reshape(1, 2)), "per_tile": per_tile}


@pytest.mark.parametrize("which", ["pooled", "per_tile"])
def test_against_the_reference_arithmetic_with_a_foreign_source(dev, be, real, oracle_sources, which):
    _, sm, tmc, quads = real
    he, max_c = oracle_sources[which]
    smd, tmcd = sm.to(dev), tmc.to(dev)
    hed, mcd = torch.from_numpy(he).to(dev), torch.from_numpy(max_c).to(dev)
    xf = synth.as_dtype(quads, torch.float32)
    rest = restated(xf.numpy(), he, max_c, sm.numpy(), tmc.numpy())

    # float32
    got = be.apply(xf.to(dev), hed, mcd, smd, tmcd)
    want = so.restore_dtype(rest, np.float32, in_0_255=True)
    err = np.abs(got.cpu().numpy() - want).reshape(len(quads), -1).max(axis=1)
    print(f"apply {which} float32: max |out - restated| = {err.max():.3e} on 0-255 (bound {TOL_255})")
    assert err.max() <= TOL_255, err
    if which == "pooled":      # (code that quietly estimated per tile would pass nothing here: the per-tile transform is grey levels away)
        per_tile = be.transform(xf.to(dev), smd, tmcd, _extra_flags=CLASSIC)
        apart = (got - per_tile).abs().flatten(1).max(dim=1).values.cpu().numpy()
        print(f"apply pooled float32: max |out - per-tile transform| per quadrant = {apart.min():.2f} ... {apart.max():.2f}")
        assert (apart > TOL_255).all(), apart
    assert same_bits(be.apply(xf.to(dev), hed, mcd, smd, tmcd, normalize_to_0_1=True).cpu(), got.cpu() / 255.0)      # (the fused /255, divided on the CPU like the reference's)

    # uint8: which half of the rule a pixel falls under is decided by the restated value alone
    got8 = be.apply(quads.to(dev), hed, mcd, smd, tmcd).cpu().numpy()
    want8 = so.restore_dtype(rest, np.uint8, in_0_255=True)
    near = np.abs(rest - np.rint(rest)) <= np.float32(TOL_255)
    share = near.reshape(len(quads), -1).mean(axis=1)
    print(f"apply {which} uint8: share of pixels within {TOL_255} of an integer per quadrant = {share.min():.4f} ... {share.max():.4f} (cap {LOOSE_SHARE})")
    assert share.max() <= LOOSE_SHARE, share
    assert got8.dtype == np.uint8 and np.array_equal(got8[~near], want8[~near])
    assert np.abs(got8.astype(np.int16) - want8.astype(np.int16))[near].max() <= 1

    # bf16 / f16 tiles: their own unit values in, the restated float cast as torch casts it
    for dt in (torch.bfloat16, torch.float16):
        xh = synth.as_dtype(quads, dt)
        rest_h = restated(xh.float().numpy(), he, max_c, sm.numpy(), tmc.numpy())
        want_h = torch.from_numpy(rest_h).to(dt)
        got_h = be.apply(xh.to(dev), hed, mcd, smd, tmcd).cpu()
        assert got_h.dtype == dt
        diff = (got_h.double() - want_h.double()).abs()
        print(f"apply {which} {dt}: max diff {diff.max().item()}, share of differing elements {(diff > 0).float().mean().item():.2e}")
        assert diff.max().item() <= HALF_BOUND[dt] and (diff > 0).float().mean().item() < HALF_SHARE, dt
    # uint8 -> bf16 / f16: the uint8 result, cast
    for dt in (torch.bfloat16, torch.float16):
        assert same_bits(be.apply(quads.to(dev), hed, mcd, smd, tmcd, out_dtype=dt).cpu(), torch.from_numpy(got8).to(dt)), dt


# ------------------------------------------------------------------------------------------------ 3. the public API
def test_pooled_estimate_and_public_apply(dev, be, real):
    imgs, sm, tmc, quads = real
    x = quads.to(dev)
    norm = Macenko(device=dev, backend="torch_hip")
    est = norm.estimate(x, pooled=True)      # (needs no fit)
    assert isinstance(est, StainEstimate) and est.stain_matrices.shape == (1, 3, 2) and est.max_concentrations.shape == (1, 2) and est.tissue_pixels is None
    he, max_c = be.compute_reference_stain_matrix(x)
    assert same_bits(est.stain_matrices[0], he) and same_bits(est.max_concentrations[0], max_c)
    with pytest.raises(ValueError, match="fit"):
        norm.apply(x, est)
    norm.fit(imgs[0:1].to(dev))
    ref = (norm._stain_matrix, norm._target_max_conc)
    out = norm.apply(x, est)
    assert out.dtype == torch.uint8 and same_bits(out, be.apply(x, he, max_c, *ref))
    second = quads[:5].flip(0).contiguous().to(dev)      # (the same estimate on another batch)
    assert same_bits(norm.apply(second, est), be.apply(second, he, max_c, *ref))
    assert same_bits(norm.apply(x, (he, max_c)), out) and same_bits(norm.apply(x, (he.reshape(1, 3, 2), max_c.reshape(1, 2))), out)
    # per tile: Macenko.estimate, and a separation that carries maxC; both give the transform
    per_tile = norm.estimate(x)
    assert per_tile.stain_matrices.shape == (24, 3, 2) and per_tile.max_concentrations.shape == (24, 2) and per_tile.tissue_pixels.shape == (24,)
    # (grey levels: no level's optical density lies within rounding of the 0.15 threshold -- level 205 gives 0.1528, 206 gives 0.1479 -- so the count is exact)
    kept = (so.optical_density(so.to_unit_float(quads.numpy())).min(axis=1) >= so.BETA).reshape(24, -1).sum(axis=1)
    assert np.array_equal(per_tile.tissue_pixels.cpu().numpy(), kept.astype(np.float32))
    want = norm.transform(x)
    assert same_bits(norm.apply(x, per_tile), want)
    sep = norm.separate(x)
    assert sep.max_concentrations is not None and same_bits(norm.apply(x, sep), want)
    # factors and own basis
    alpha, beta = factors(24, dev)
    assert same_bits(norm.apply(x, per_tile, alpha=alpha, beta=beta), be.augment(x, alpha, beta, *ref))
    unfitted = Macenko(device=dev, backend="torch_hip")
    own = unfitted.apply(x, per_tile, alpha=alpha, beta=beta, own_basis=True)
    assert same_bits(own, be.augment(x, alpha, beta))
    assert same_bits(unfitted.apply(x, StainEstimate(per_tile.stain_matrices, None, None), alpha=alpha, beta=beta, own_basis=True), own)
    # the output type follows normalize_to_0_1 / output_dtype as transform's does
    unit = Macenko(device=dev, backend="torch_hip", normalize_to_0_1=True, precision="fast")
    unit.fit(imgs[0:1].to(dev))
    out01 = unit.apply(x, est)
    assert out01.dtype == torch.float32 and same_bits(out01.cpu(), out.cpu().float() / 255.0)
    half = Macenko(device=dev, backend="torch_hip", output_dtype=torch.bfloat16)
    half.fit(imgs[0:1].to(dev))
    assert same_bits(half.apply(x, est), out.to(torch.bfloat16))
    xf = synth.as_dtype(quads, torch.float32).to(dev)
    assert norm.apply(xf, est).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 4. degenerate tiles and sources
def fold_restated(x255: np.ndarray, he: np.ndarray, max_c: np.ndarray, sm: np.ndarray, tmc: np.ndarray) -> np.ndarray:
    """The transform's fold for ONE tile, (3, P) grey levels 0..255 in, float32 0-255 out after its clamp: scale = tmc / maxC in float32 (a zero
    maxC: infinite), M = SM diag(scale) pinv(HE) and k = log2(240) (1 - row sums) formed in float64 and rounded to float32, x = k + M L with
    L = log2(level + 1), rgb = min(max(2^x, 0), 255) with a NaN clamped to 0 (fmaxf(NaN, 0) = 0)."""
    with np.errstate(all="ignore"):
        pinv = np.linalg.pinv(he.astype(np.float64)).astype(np.float32).astype(np.float64)
        s = (tmc.astype(np.float32) / max_c.astype(np.float32)).astype(np.float64)
        smd = sm.astype(np.float64)
        m = ((smd[:, 0:1] * s[0]) * pinv[0][None, :] + (smd[:, 1:2] * s[1]) * pinv[1][None, :]).astype(np.float32)
        k = (7.90689059560851852932 * (1.0 - m.astype(np.float64).sum(axis=1))).astype(np.float32)
        lv = np.log2(x255.astype(np.float32) + np.float32(1.0)).astype(np.float32)
        xx = k[:, None] + m[:, 0:1] * lv[0] + m[:, 1:2] * lv[1] + m[:, 2:3] * lv[2]
        rgb = np.exp2(xx.astype(np.float32))
        return np.where(np.isnan(rgb), np.float32(0), np.clip(rgb, np.float32(0), np.float32(255))).astype(np.float32)


def test_degenerate_tiles_and_sources_stay_defined(dev, be, real):
    """An all-white tile and a constant tile next to tissue; a source maxC with a zero entry (infinite scale, as the transform); a rank-1 HE
    (second column zero: the rank rule drops it).  The tissue tiles' outputs do not change, the degenerate ones are the fold's clamp-then-cast."""
    _, sm, tmc, quads = real
    smd, tmcd = sm.to(dev), tmc.to(dev)
    tissue = quads[:2]
    white = torch.full((1, 3, 512, 512), 255, dtype=torch.uint8)
    pink = torch.tensor([217, 140, 191], dtype=torch.uint8).view(1, 3, 1, 1).expand(1, 3, 512, 512)
    x8 = torch.cat([tissue, white, pink, tissue]).contiguous()      # tiles 4, 5: tissue again, with a degenerate SOURCE
    for dt in (torch.uint8, torch.float32):
        x = synth.as_dtype(x8, dt).to(dev)
        est = be.estimate(x)
        he, max_c = est["he"].clone(), est["max_c"].clone()
        assert torch.isfinite(he).all()
        he[2], max_c[2] = he[0], max_c[0]      # (the white and the constant tile with a neighbour's basis: what a slide-level source is for)
        he[3], max_c[3] = he[1], max_c[1]
        max_c[4, 0] = 0.0                      # an infinite H scale
        he[5, :, 1] = 0.0                      # a rank-1 basis
        got = be.apply(x, he, max_c, smd, tmcd)
        # the tissue tiles next to them: unchanged, bit for bit (and they are the transform)
        alone = be.apply(x[:2].contiguous(), he[:2], max_c[:2], smd, tmcd)
        assert same_bits(got[:2], alone) and same_bits(alone, be.transform(x[:2].contiguous(), smd, tmcd, _extra_flags=CLASSIC)), dt
        hen, mcn = he.cpu().numpy(), max_c.cpu().numpy()
        # white / constant tiles: one colour in, one colour out, the fold's value
        for i in (2, 3):
            want = fold_restated(x8[i].reshape(3, -1).numpy(), hen[i], mcn[i], sm.numpy(), tmc.numpy())
            out = got[i].reshape(3, -1).cpu()
            assert (out == out[:, :1]).all(), (dt, i)
            if dt == torch.uint8:
                near = np.abs(want - np.rint(want)) <= TOL_255
                assert np.array_equal(out.numpy()[~near], np.trunc(want).astype(np.uint8)[~near]) and np.abs(out.numpy().astype(np.int16) - np.trunc(want).astype(np.int16)).max() <= 1, i
            else:
                assert np.abs(out.numpy() - want).max() <= TOL_255, i
        # zero maxC: every value of the fold is infinite or NaN, the output saturated -- exactly the clamp-then-cast of the fold
        want = fold_restated(x8[4].reshape(3, -1).numpy(), hen[4], mcn[4], sm.numpy(), tmc.numpy())
        assert np.isin(want, (0.0, 255.0)).all()
        out = got[4].reshape(3, -1).cpu().numpy()
        assert np.array_equal(out.astype(np.float32), want), dt
        # rank-1 HE: lstsq drops the second singular value, the E concentration is exactly 0
        rest = restated(x8[5:6].numpy(), hen[5:6], mcn[5:6], sm.numpy(), tmc.numpy())[0]
        assert np.isfinite(rest).all()
        out = got[5].cpu().numpy()
        if dt == torch.uint8:
            near = np.abs(rest - np.rint(rest)) <= TOL_255
            want8 = so.restore_dtype(rest, np.uint8, in_0_255=True)
            assert np.array_equal(out[~near], want8[~near]) and np.abs(out.astype(np.int16) - want8.astype(np.int16)).max() <= 1
        else:
            assert np.abs(out - rest).max() <= TOL_255
        # own basis with the same sources: defined as well (finite factors, finite output)
        alpha, beta = factors(6, dev)
        own = be.apply(x, he, None, alpha=alpha, beta=beta)
        assert torch.isfinite(own.float()).all(), dt


# ------------------------------------------------------------------------------------------------ 5. graph capture, errors that reach the device side
def test_graph_replay_reads_new_images_source_and_factors(dev, be, real):
    _, sm, tmc, quads = real
    sm, tmc = sm.to(dev), tmc.to(dev)
    first = synth.as_dtype(quads[:8], torch.float32).to(dev)
    second = synth.as_dtype(quads[8:16], torch.float32).to(dev)
    e1, e2 = be.estimate(first), be.estimate(second)
    a1, b1 = factors(8, dev, seed=1)
    a2, b2 = factors(8, dev, seed=2)
    for ref in ((), (sm, tmc)):
        x, he, mc, alpha, beta = first.clone(), e1["he"].clone(), e1["max_c"].clone(), a1.clone(), b1.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                be.apply(x, he, mc, *ref, alpha=alpha, beta=beta)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = be.apply(x, he, mc, *ref, alpha=alpha, beta=beta)
        x.copy_(second)
        he.copy_(e2["he"])
        mc.copy_(e2["max_c"])
        alpha.copy_(a2)
        beta.copy_(b2)
        g.replay()
        torch.cuda.synchronize()
        want = be.apply(second, e2["he"], e2["max_c"], *ref, alpha=a2, beta=b2)
        assert same_bits(out, want), len(ref)
        assert same_bits(want, be.augment(second, a2, b2, *ref)), len(ref)


def test_c_abi_errors_and_success(dev, real):
    _, sm, tmc, _ = real
    lib = _native.require()
    x = synth.as_dtype(synth.he_batch(4, 64, 64, seed0=5000), torch.float32).to(dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    out = torch.empty_like(x)
    he, mc = torch.rand(4, 3, 2, device=dev) + 0.1, torch.ones(4, 2, device=dev)
    ab = torch.ones(4, 2, device=dev)
    smd, tmcd = sm.to(dev), tmc.to(dev)

    def call(n_sources=4, mc_ptr=mc.data_ptr(), a=None, b=None, s=smd.data_ptr(), t=tmcd.data_ptr(), flags=0):
        return lib.sx_macenko_apply(x.data_ptr(), out.data_ptr(), f32, 4, 64, 64, he.data_ptr(), mc_ptr, n_sources, a, b, s, t, flags, _native.stream_ptr(dev))

    assert call(n_sources=2) == _native.SX_ERR_BAD_ARG
    assert call(s=None) == _native.SX_ERR_BAD_ARG
    assert call(a=ab.data_ptr()) == _native.SX_ERR_BAD_ARG
    assert call(s=None, t=None) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_SAMPLED) == _native.SX_ERR_BAD_ARG
    assert call() == _native.SX_OK
    assert call(n_sources=1, flags=CLASSIC) == _native.SX_OK
    assert call(mc_ptr=None, a=ab.data_ptr(), b=ab.data_ptr(), s=None, t=None) == _native.SX_OK
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
