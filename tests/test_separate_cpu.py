"""Stain separation without a GPU: the entry point is exported by both libraries, its argument checks at the C ABI (they return
before anything is enqueued), and Macenko.separate's validation, which runs before any GPU work."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest
import torch

import stainx_amd
from stainx_amd import Macenko, StainSeparation, _native

ROOT = Path(__file__).resolve().parents[1]


def test_exported_by_both_libraries_and_declared():
    assert "sx_macenko_separate" in _native.SIGNATURES
    for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
        assert hasattr(ctypes.CDLL(str(path)), "sx_macenko_separate"), path
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    decl = re.search(r"int sx_macenko_separate\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_native.SIGNATURES["sx_macenko_separate"][1])


def test_public_name():
    assert "StainSeparation" in stainx_amd.__all__
    assert stainx_amd.StainSeparation is StainSeparation
    assert StainSeparation._fields == ("hematoxylin", "eosin", "concentrations", "stain_matrices", "max_concentrations")


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_macenko_workspace_bytes_for(f32, 2, 64, 64, _native.MACENKO_CLASSIC))
    fake = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)

    def call(stains=fake, conc=fake, sm=None, tmc=None, flags=0, nbytes=need, dtype=f32, images=fake):
        return lib.sx_macenko_separate(images, stains, conc, dtype, 2, 64, 64, sm, tmc, None, None, flags, fake, nbytes, None)

    assert call(stains=None, conc=None) == _native.SX_ERR_BAD_ARG
    assert call(sm=fake) == _native.SX_ERR_BAD_ARG and "both" in _native.last_error()
    assert call(tmc=fake) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_SAMPLED) == _native.SX_ERR_BAD_ARG
    for bit in (_native.MACENKO_TWO_PASS, _native.MACENKO_NO_TIE_SHORTCUT, _native.MACENKO_NO_CODES):
        assert call(flags=bit) == _native.SX_ERR_BAD_ARG
    assert call(flags=_native.MACENKO_OUT_BF16) == _native.SX_ERR_BAD_ARG      # (uint8 input only)
    assert call(nbytes=need - 1) == _native.SX_ERR_WORKSPACE
    assert call(images=None) == _native.SX_ERR_BAD_ARG


def test_method_validation_before_gpu_work():
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    norm = Macenko(device="cuda")
    with pytest.raises(ValueError, match="fit"):
        norm.separate(x, own_basis=False)
    with pytest.raises(ValueError, match="approximate"):
        Macenko(device="cuda", precision="sampled").separate(x)
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="C=3"):
            norm.separate(bad)
    with pytest.raises(ValueError, match="stains, concentrations"):
        norm.separate(x, stains=False, concentrations=False)
