"""Slide-level Macenko without a GPU: sx_macenko_estimate and sx_macenko_apply are exported by both libraries and declared, their
argument checks at the C ABI return before anything is enqueued, and Macenko.estimate / Macenko.apply validate before any GPU work."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest
import torch

import stainx_amd
from stainx_amd import Macenko, StainEstimate, StainSeparation, _native

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("sx_macenko_estimate", "sx_macenko_apply")


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name in NAMES:
        assert name in _native.SIGNATURES
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(r"int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name
    assert len(_native.SIGNATURES["sx_macenko_estimate"][1]) == 12 and len(_native.SIGNATURES["sx_macenko_apply"][1]) == 15
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)


def test_public_name():
    assert "StainEstimate" in stainx_amd.__all__
    assert stainx_amd.StainEstimate is StainEstimate
    assert StainEstimate._fields == ("stain_matrices", "max_concentrations", "tissue_pixels")


def test_apply_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    fake = 1 << 40      # (never dereferenced: every call below fails its checks first)

    def call(images=fake, out=fake, dtype=f32, n=4, he=fake, max_c=fake, n_sources=4, alpha=None, beta=None, sm=fake, tmc=fake, flags=0):
        return lib.sx_macenko_apply(images, out, dtype, n, 64, 64, he, max_c, n_sources, alpha, beta, sm, tmc, flags, None)

    bad = _native.SX_ERR_BAD_ARG
    assert call(images=None) == bad
    assert call(out=None) == bad
    assert call(he=None) == bad
    assert call(n=0) == bad
    assert call(n_sources=2) == bad and "n_sources" in _native.last_error()
    assert call(n_sources=0) == bad
    assert call(sm=None) == bad and "both" in _native.last_error()      # exactly one pointer of a pair
    assert call(tmc=None) == bad
    assert call(alpha=fake) == bad and "both" in _native.last_error()
    assert call(beta=fake) == bad
    assert call(sm=None, tmc=None) == bad and "own basis" in _native.last_error()      # own basis without factors
    assert call(max_c=None) == bad      # (null only in own-basis mode)
    assert call(flags=_native.MACENKO_SAMPLED) == bad
    for bit in (_native.MACENKO_NO_TIE_SHORTCUT, _native.MACENKO_SPEC_FAIL, _native.MACENKO_TWO_PASS, _native.MACENKO_FUSE, _native.MACENKO_RESIDENT,
                _native.MACENKO_NO_CODES, 1 << 20):
        assert call(flags=bit) == bad, bit
    assert call(flags=_native.MACENKO_OUT_BF16) == bad      # (uint8 input only)
    assert call(flags=_native.MACENKO_OUT_F16) == bad
    assert call(dtype=u8, flags=_native.MACENKO_OUT_BF16 | _native.MACENKO_OUT_F16) == bad
    assert call(dtype=17) == _native.SX_ERR_DTYPE
    # the diagnostic build takes the same set of flags: its diagnostic bits belong to the transform
    diag = _native.require_diag()
    assert diag.sx_macenko_apply(fake, fake, f32, 4, 64, 64, fake, fake, 4, None, None, fake, fake, _native.MACENKO_TWO_PASS, None) == bad


def test_estimate_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_macenko_workspace_bytes_for(f32, 2, 64, 64, _native.MACENKO_CLASSIC))
    fake = 1 << 40      # (256-byte aligned, never dereferenced)

    def call(images=fake, he=fake, max_c=fake, tissue=None, flags=0, nbytes=need, ws=fake):
        return lib.sx_macenko_estimate(images, f32, 2, 64, 64, he, max_c, tissue, flags, ws, nbytes, None)

    bad = _native.SX_ERR_BAD_ARG
    assert call(images=None) == bad
    assert call(he=None) == bad
    assert call(max_c=None) == bad
    for bit in (_native.MACENKO_SAMPLED, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16, _native.MACENKO_TWO_PASS,
                _native.MACENKO_NO_TIE_SHORTCUT, _native.MACENKO_NO_CODES):
        assert call(flags=bit) == bad, bit
    assert call(nbytes=need - 1) == _native.SX_ERR_WORKSPACE
    assert call(ws=None) == _native.SX_ERR_WORKSPACE
    assert call(ws=fake + 8) == _native.SX_ERR_WORKSPACE


def test_method_validation_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    he, mc = torch.zeros(4, 3, 2), torch.ones(4, 2)
    ab = torch.ones(4, 2)
    norm = Macenko(device="cuda")
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):      # (transform's own text)
        norm.apply(x, (he, mc))
    with pytest.raises(ValueError, match="approximate"):
        Macenko(device="cuda", precision="sampled").estimate(x)
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="C=3"):
            norm.estimate(bad)
        with pytest.raises(ValueError, match="C=3"):
            norm.apply(bad, (he, mc), alpha=ab, beta=ab, own_basis=True)
    with pytest.raises(ValueError, match="factors"):
        norm.apply(x, (he, mc), own_basis=True)
    with pytest.raises(ValueError, match="together"):
        norm.apply(x, (he, mc), alpha=ab, own_basis=True)
    # a fitted normaliser (the slots filled by hand: no GPU here), so that the source's shapes are what is refused
    norm._stain_matrix, norm._target_max_conc, norm._is_fitted = torch.zeros(3, 2), torch.ones(2), True
    for src in ((torch.zeros(2, 3, 2), torch.ones(2, 2)), (torch.zeros(4, 2, 3), mc), (torch.zeros(6), torch.ones(2)), (he, torch.ones(1, 2)),
                (he, torch.ones(4, 3)), (torch.zeros(3, 2), torch.ones(4, 2)), (torch.zeros(1, 3, 2), torch.ones(4, 2))):
        with pytest.raises(ValueError, match="shape"):
            norm.apply(x, src)
    with pytest.raises(ValueError, match="source must be"):
        norm.apply(x, he)
    with pytest.raises(ValueError, match="max_concentrations"):
        norm.apply(x, StainSeparation(None, None, None, he, None))      # (a separation in its own basis carries no maxC)
    with pytest.raises(ValueError, match="max_concentrations"):
        norm.apply(x, StainEstimate(he, None, None))
    for name in ("alpha", "beta"):
        with pytest.raises(ValueError, match=name):
            norm.apply(x, (he, mc), **{"alpha": ab, "beta": ab, name: torch.ones(3, 2)})
