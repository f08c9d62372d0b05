"""Stain augmentation without a GPU: the entry point is exported by both libraries, its argument checks at the C ABI (they
return before anything is enqueued), and MacenkoAugment's validation, which runs before any GPU work."""
from __future__ import annotations

import ctypes

import pytest
import torch

import stainx_amd
from stainx_amd import MacenkoAugment, _native


def test_exported_by_both_libraries():
    assert "sx_macenko_augment" in _native.SIGNATURES
    for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
        assert hasattr(ctypes.CDLL(str(path)), "sx_macenko_augment"), path


def test_public_name():
    assert "MacenkoAugment" in stainx_amd.__all__
    assert stainx_amd.MacenkoAugment is MacenkoAugment


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_macenko_workspace_bytes_for(f32, 2, 64, 64, _native.MACENKO_CLASSIC))
    fake = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)

    def call(alpha=fake, beta=fake, sm=None, tmc=None, flags=0, nbytes=need, dtype=f32):
        return lib.sx_macenko_augment(fake, fake, dtype, 2, 64, 64, alpha, beta, sm, tmc, flags, fake, nbytes, None)

    assert call(alpha=None) == _native.SX_ERR_BAD_ARG
    assert call(beta=None) == _native.SX_ERR_BAD_ARG
    assert call(sm=fake) == _native.SX_ERR_BAD_ARG and "both" in _native.last_error()
    assert call(tmc=fake) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_SAMPLED) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_TWO_PASS) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_OUT_BF16) == _native.SX_ERR_BAD_ARG      # (uint8 input only)
    assert call(nbytes=need - 1) == _native.SX_ERR_WORKSPACE
    assert lib.sx_macenko_augment(None, fake, f32, 2, 64, 64, fake, fake, None, None, 0, fake, need, None) == _native.SX_ERR_BAD_ARG


@pytest.mark.parametrize("kwargs", [{"sigma1": 1.0}, {"sigma1": -0.1}, {"sigma1": float("nan")}, {"sigma2": -0.5}, {"sigma2": float("inf")}, {"device": "cpu"}])
def test_module_validation(kwargs):
    with pytest.raises(ValueError):
        MacenkoAugment(**kwargs)


def test_module_validation_before_gpu_work():
    with pytest.raises(ValueError, match="not both"):
        MacenkoAugment(reference=torch.zeros(1, 3, 8, 8, dtype=torch.uint8), normalizer=stainx_amd.Macenko(device="cuda"))
    with pytest.raises(ValueError, match="fitted"):
        MacenkoAugment(normalizer=stainx_amd.Macenko(device="cuda"))
    with pytest.raises(ValueError, match="Macenko"):
        MacenkoAugment(normalizer=stainx_amd.Reinhard(device="cuda"))
    with pytest.raises(ValueError, match="CUDA"):
        MacenkoAugment(reference=torch.zeros(1, 3, 8, 8, dtype=torch.uint8))      # a CPU reference and no device
    m = MacenkoAugment(0.1, 0.1)
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(8, 8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="C=3"):
            m(bad)
    with pytest.raises(ValueError, match="CUDA"):
        m(torch.zeros(2, 3, 8, 8))      # a CPU tensor and no device


def test_sample_factors_on_the_host():
    m = MacenkoAugment(0.2, 0.1, generator=torch.Generator().manual_seed(0))
    alpha, beta = m.sample_factors(4096, "cpu")
    assert alpha.shape == beta.shape == (4096, 2) and alpha.dtype == beta.dtype == torch.float32
    assert 0.8 - 1e-6 <= alpha.min().item() and alpha.max().item() <= 1.2 + 1e-6
    assert -0.1 - 1e-6 <= beta.min().item() and beta.max().item() <= 0.1 + 1e-6
    again = MacenkoAugment(0.2, 0.1, generator=torch.Generator().manual_seed(0)).sample_factors(4096, "cpu")
    assert torch.equal(alpha, again[0]) and torch.equal(beta, again[1])
    a0, b0 = MacenkoAugment(0.0, 0.0).sample_factors(8, "cpu")
    assert torch.equal(a0, torch.ones(8, 2)) and torch.equal(b0, torch.zeros(8, 2))
