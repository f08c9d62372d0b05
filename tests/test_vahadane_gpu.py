"""The Vahadane estimate and the percentile call on the GPU: the basis against the float64 restatement (tests/_vahadane_numpy.py) after 1, 8
and 30 rounds, per tile and pooled, masked and not, for the five element types; maxC bit for bit the nearest-rank percentile of the
concentrations ``separate`` writes; the bit-for-bit identities the fixed reduction order promises; and the degenerate groups.

Crops of the six real images: (3, 45 x 67) -- odd width, no wide packs, one work item per tile --, (2, 128 x 128) and (6, 224 x 224) -- four
work items per tile."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Vahadane, stain_basis, synth, tissue_mask
from tests import _vahadane_numpy as vn
from tests.conftest import TORCH_DTYPES
from tests.test_tissue_mask_gpu import unaligned_copy

pytestmark = pytest.mark.gpu

CASES = {"odd": (3, 45, 67), "mid": (2, 128, 128), "big": (6, 224, 224)}
DTYPES = ["u8", "f32", "bf16", "f16", "f64"]
# Largest |he - float64 restatement| measured on an MI355X over every combination test_basis_against_float64 runs: 8.4e-6 (float32 tiles
# of 45 x 67 after 30 rounds; 7.5e-8 .. 2.9e-6 elsewhere: DESIGN.md 4p); the bound is four times that.  It covers the float32 coding step
# and the float32 per-thread partial sums.
HE_BOUND = 4 * 8.4e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def crop_u8(case: str) -> torch.Tensor:
    n, h, w = CASES[case]
    return torch.from_numpy(vn.real_images()[:n, :, 300:300 + h, 400:400 + w].copy())


def tiles(case: str, name: str) -> torch.Tensor:
    return synth.as_dtype(crop_u8(case), TORCH_DTYPES[name])


def as_numpy(x: torch.Tensor) -> np.ndarray:
    return x.numpy() if x.dtype == torch.uint8 else x.double().numpy()


def explicit_mask(case: str) -> torch.Tensor:
    """Tile 0: a random half; tile 1: fully masked out; tile 2 (where there is one): a single masked-in pixel; further tiles: a random half."""
    n, h, w = CASES[case]
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(n, h, w, generator=gen) < 0.5).to(torch.uint8) * 7      # (non-zero = in)
    mask[1] = 0
    if n > 2:
        mask[2] = 0
        mask[2, h // 2, w // 3] = 1
    return mask


def masks_of(case: str, x_dev: torch.Tensor) -> dict:
    return {"none": None, "luminosity": tissue_mask(x_dev)[0], "explicit": explicit_mask(case).to(x_dev.device)}


def init_f64() -> np.ndarray:
    return stain_basis("he")[:, :2].double().numpy()


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ 1. the basis against the float64 restatement
@pytest.mark.parametrize("iterations", [1, 8, 30])
@pytest.mark.parametrize("case,name", [("odd", name) for name in DTYPES] + [("mid", "u8"), ("mid", "f32"), ("big", "u8"), ("big", "bf16")])
def test_basis_against_float64(dev, case, name, iterations):
    x = tiles(case, name)
    x_dev = x.to(dev)
    norm = Vahadane(device=dev, iterations=iterations, mask=None)
    worst = 0.0
    for kind, mask in masks_of(case, x_dev).items():
        mask_np = None if mask is None else mask.cpu().numpy()
        for pooled in (False, True):
            got = norm.estimate(x_dev, pooled=pooled, mask=mask)
            want = vn.estimate(as_numpy(x), mask_np, pooled=pooled, init=init_f64(), lam=0.1, iterations=iterations)
            he = got.stain_matrices.cpu().double().numpy()
            assert he.shape == want.shape
            assert np.array_equal(np.isnan(he), np.isnan(want)), (kind, pooled)
            count = (np.ones(x.shape[0]) * x.shape[2] * x.shape[3]) if mask_np is None else (mask_np.reshape(x.shape[0], -1) != 0).sum(axis=1)
            if pooled:
                assert got.tissue_pixels is None
            else:
                assert got.tissue_pixels.dtype == torch.float32 and np.array_equal(got.tissue_pixels.cpu().numpy(), count.astype(np.float32))
            if not np.isnan(want).all():
                worst = max(worst, float(np.nanmax(np.abs(he - want))))
    print(f"vahadane basis {case} {name} iterations={iterations}: max |he - float64| = {worst:.3e}")
    assert worst <= HE_BOUND, worst


# ------------------------------------------------------------------ 2. maxC is exact
def wanted_max_c(conc: np.ndarray, mask_np: np.ndarray | None, pooled: bool) -> np.ndarray:
    n = conc.shape[0]
    keep = np.ones((n, conc.shape[2] * conc.shape[3]), dtype=bool) if mask_np is None else mask_np.reshape(n, -1) != 0
    flat = conc.reshape(n, 2, -1)
    groups = [list(range(n))] if pooled else [[t] for t in range(n)]
    out = np.full((len(groups), 2), np.nan, dtype=np.float32)
    for r, members in enumerate(groups):
        for s in range(2):
            values = np.concatenate([flat[t, s][keep[t]] for t in members])
            if values.size:
                out[r, s] = so.nearest_rank(values, 99)
    return out


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("case", ["odd", "big"])
def test_max_concentrations_are_the_exact_percentiles(dev, case, name):
    x_dev = tiles(case, name).to(dev)
    norm = Vahadane(device=dev, iterations=4, mask=None)
    given = stain_basis("he")[:, :2].to(dev)
    for kind, mask in masks_of(case, x_dev).items():
        mask_np = None if mask is None else mask.cpu().numpy()
        for pooled in (False, True):
            est = norm.estimate(x_dev, pooled=pooled, mask=mask)
            for he, own in ((est.stain_matrices, est.max_concentrations), (given, None)):
                conc = norm.separate(x_dev, source=(he, None), own_basis=True, stains=False, concentrations=True, mask=mask).concentrations.cpu().numpy()
                want = wanted_max_c(conc, mask_np, pooled)
                if he.dim() == 3 and not pooled:      # (a tile without an estimate: NaN basis, NaN percentiles)
                    want[np.isnan(he.cpu().numpy()).any(axis=(1, 2))] = np.nan
                got = norm.max_concentrations(x_dev, he, pooled=pooled, mask=mask).cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, pooled, own is None, got, want)
                if own is not None:
                    assert np.array_equal(own.cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, pooled, own, want)


# ------------------------------------------------------------------ 3. identities, bit for bit
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
@pytest.mark.parametrize("case", ["odd", "big"])
def test_identities(dev, case, name):
    x_dev = tiles(case, name).to(dev)
    n = x_dev.shape[0]
    norm = Vahadane(device=dev, iterations=6, mask=None)
    for kind, mask in masks_of(case, x_dev).items():
        first = norm.estimate(x_dev, mask=mask)
        again = norm.estimate(x_dev, mask=mask)
        assert same_bits(first.stain_matrices, again.stain_matrices) and same_bits(first.max_concentrations, again.max_concentrations), kind
        for t in range(n):
            alone_mask = None if mask is None else mask[t:t + 1]
            alone = norm.estimate(x_dev[t:t + 1], mask=alone_mask)
            assert same_bits(alone.stain_matrices, first.stain_matrices[t:t + 1]) and same_bits(alone.max_concentrations, first.max_concentrations[t:t + 1]), (kind, t)
            pooled = norm.estimate(x_dev[t:t + 1], mask=alone_mask, pooled=True)
            assert same_bits(pooled.stain_matrices, alone.stain_matrices) and same_bits(pooled.max_concentrations, alone.max_concentrations), (kind, t)
            moved = norm.estimate(unaligned_copy(x_dev[t:t + 1]), mask=alone_mask)      # (the scalar path visits the pixels in the packs' order)
            assert same_bits(moved.stain_matrices, alone.stain_matrices) and same_bits(moved.max_concentrations, alone.max_concentrations), (kind, t)
        engine = norm._get_backend_impl()
        bare = engine.vahadane_estimate(x_dev, stain_basis("he")[:, :2], regularizer=0.1, iterations=6, masked=mask is not None, mask=mask, max_conc=False)
        assert bare["max_c"] is None and same_bits(bare["he"], first.stain_matrices), kind
    ones = torch.ones((n, x_dev.shape[2], x_dev.shape[3]), dtype=torch.uint8, device=dev)
    for pooled in (False, True):
        plain, under = norm.estimate(x_dev, pooled=pooled), norm.estimate(x_dev, pooled=pooled, mask=ones)
        assert same_bits(plain.stain_matrices, under.stain_matrices) and same_bits(plain.max_concentrations, under.max_concentrations), pooled
    if name != "u8":      # NaN under masked-out pixels changes nothing
        mask = explicit_mask(case).to(dev)
        spoiled = x_dev.clone()
        spoiled[(mask == 0).unsqueeze(1).expand_as(spoiled)] = float("nan")
        for pooled in (False, True):
            clean, dirty = norm.estimate(x_dev, pooled=pooled, mask=mask), norm.estimate(spoiled, pooled=pooled, mask=mask)
            assert same_bits(clean.stain_matrices, dirty.stain_matrices) and same_bits(clean.max_concentrations, dirty.max_concentrations), pooled


# ------------------------------------------------------------------ 4. degenerate groups
def test_degenerate_groups(dev):
    x = crop_u8("odd")
    x_dev = x.to(dev)
    mask = explicit_mask("odd").to(dev)
    norm = Vahadane(device=dev, mask=None)
    est = norm.estimate(x_dev, mask=mask)
    he, max_c = est.stain_matrices.cpu(), est.max_concentrations.cpu()
    assert torch.isnan(he[1]).all() and torch.isnan(max_c[1]).all() and est.tissue_pixels[1].item() == 0      # fully masked out
    assert est.tissue_pixels[2].item() == 1 and torch.isfinite(he[2]).all() and torch.isfinite(max_c[2]).all()      # a single pixel
    assert torch.allclose((he[2].double() ** 2).sum(dim=0), torch.ones(2, dtype=torch.float64), atol=1e-6) and (he[2] >= 0).all()
    out = norm.fit(x_dev).transform(x_dev, mask=mask)
    assert out.dtype == torch.uint8 and torch.equal(out[1].cpu(), x[1])      # the tile without an estimate: copied byte for byte
    assert torch.equal(out.cpu()[(mask.cpu() == 0).unsqueeze(1).expand_as(x)], x[(mask.cpu() == 0).unsqueeze(1).expand_as(x)])
    glass = torch.full((1, 3, 45, 67), 255, dtype=torch.uint8, device=dev)      # optical density below zero: every code is 0, the columns stay
    kept = norm.estimate(glass).stain_matrices.cpu()[0]
    assert torch.allclose(kept, stain_basis("he")[:, :2], atol=1.2e-7, rtol=0)
