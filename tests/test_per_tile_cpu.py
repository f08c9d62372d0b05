"""Per-tile Reinhard / histogram matching without a GPU: the new entry points are exported by both libraries and declared, their argument
checks at the C ABI return before anything is enqueued, the workspace sizes behave, and the classes validate before any GPU work."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest
import torch

import stainx_amd
from stainx_amd import ColorStatistics, HistogramMatching, Reinhard, _native

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_reinhard_tile_stats": 10, "sx_reinhard_transform_tiles": 13, "sx_reinhard_apply_stats": 12, "sx_hm_transform_tiles": 13}
SIZES = {"sx_reinhard_tiles_workspace_bytes": 4, "sx_hm_tiles_workspace_bytes": 3}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for names, restype in ((CALLS, "int"), (SIZES, "size_t")):
        for name, params in names.items():
            assert name in _native.SIGNATURES
            assert len(_native.SIGNATURES[name][1]) == params, name
            for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
                assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
            decl = re.search(restype + " " + name + r"\((.*?)\);", header, flags=re.S).group(1)
            decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
            assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1


def test_public_names_and_modes():
    assert "ColorStatistics" in stainx_amd.__all__
    assert stainx_amd.ColorStatistics is ColorStatistics
    assert ColorStatistics._fields == ("mean", "std")
    for cls in (Reinhard, HistogramMatching):
        with pytest.raises(ValueError, match="statistics"):
            cls(device="cuda", statistics="nope")
        assert cls(device="cuda").statistics == "batch"      # the default is the pooled path
        assert cls(device="cuda", statistics="tile").statistics == "tile"
    assert HistogramMatching(device="cuda", channel_axis=-1, statistics="tile").channel_axis == -1


def test_reinhard_tile_calls_reject_bad_arguments_before_any_launch():
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]
    need = int(lib.sx_reinhard_tiles_workspace_bytes(f32, 4, 64, 64))

    def stats(images=FAKE, dtype=f32, n=4, mean=FAKE, std=FAKE, ws=FAKE, nbytes=need):
        return lib.sx_reinhard_tile_stats(images, dtype, n, 64, 64, mean, std, ws, nbytes, None)

    def transform(images=FAKE, out=FAKE, dtype=f32, n=4, rm=FAKE, rs=FAKE, mean=None, std=None, ws=FAKE, nbytes=need):
        return lib.sx_reinhard_transform_tiles(images, out, dtype, n, 64, 64, rm, rs, mean, std, ws, nbytes, None)

    assert stats(images=None) == BAD
    assert stats(mean=None) == BAD
    assert stats(std=None) == BAD
    assert stats(n=0) == BAD and stats(n=-3) == BAD
    assert stats(dtype=17) == DTYPE
    assert stats(nbytes=need - 1) == WORKSPACE
    assert stats(ws=None) == WORKSPACE
    assert stats(ws=FAKE + 8) == WORKSPACE

    assert transform(images=None) == BAD
    assert transform(out=None) == BAD
    assert transform(rm=None) == BAD
    assert transform(rs=None) == BAD
    assert transform(n=0) == BAD
    assert transform(mean=FAKE) == BAD and "both" in _native.last_error()      # exactly one of the two outputs
    assert transform(std=FAKE) == BAD
    assert transform(dtype=17) == DTYPE
    assert transform(nbytes=need - 1) == WORKSPACE
    assert transform(ws=None) == WORKSPACE
    assert transform(ws=FAKE + 8) == WORKSPACE
    # the diagnostic build checks the same way
    diag = _native.require_diag()
    assert diag.sx_reinhard_transform_tiles(FAKE, FAKE, f32, 4, 64, 64, FAKE, FAKE, FAKE, None, FAKE, need, None) == BAD


def test_reinhard_apply_stats_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    f32 = _native.DTYPE_CODES[torch.float32]

    def call(images=FAKE, out=FAKE, dtype=f32, n=4, mean=FAKE, std=FAKE, n_sources=4, rm=FAKE, rs=FAKE):
        return lib.sx_reinhard_apply_stats(images, out, dtype, n, 64, 64, mean, std, n_sources, rm, rs, None)

    assert call(images=None) == BAD
    assert call(out=None) == BAD
    assert call(mean=None) == BAD
    assert call(std=None) == BAD
    assert call(rm=None) == BAD
    assert call(rs=None) == BAD
    assert call(n=0) == BAD
    for n_sources in (0, 2, 3, 5, -1):
        assert call(n_sources=n_sources) == BAD and "n_sources" in _native.last_error(), n_sources
    assert call(dtype=17) == DTYPE
    assert call(dtype=17, n_sources=1) == DTYPE


def test_hm_tiles_rejects_bad_arguments_before_any_launch():
    lib = _native.require()
    u8 = _native.DTYPE_CODES[torch.uint8]
    need = int(lib.sx_hm_tiles_workspace_bytes(4, 64, 64))

    def call(images=FAKE, out=FAKE, dtype=u8, n=4, last=0, ref=FAKE, counts=None, lut=None, ws=FAKE, nbytes=need):
        return lib.sx_hm_transform_tiles(images, out, dtype, n, 64, 64, last, ref, counts, lut, ws, nbytes, None)

    assert call(images=None) == BAD
    assert call(out=None) == BAD
    assert call(ref=None) == BAD
    assert call(n=0) == BAD and call(n=-1) == BAD
    assert call(dtype=17) == DTYPE
    assert call(last=1, dtype=17) == DTYPE
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(nbytes=int(lib.sx_hm_workspace_bytes(4, 64, 64))) == WORKSPACE      # (the pooled size does not do)
    assert call(ws=None) == WORKSPACE
    assert call(ws=FAKE + 8) == WORKSPACE


def test_tile_workspace_sizes():
    lib = _native.require()
    for dtype in _native.DTYPE_CODES.values():
        for h, w in ((1, 1), (33, 47), (224, 224), (512, 512)):
            assert lib.sx_reinhard_tiles_workspace_bytes(dtype, 0, h, w) == 0
            last = 0
            for n in (1, 2, 3, 5, 16, 64, 100, 4096, 5000):
                size = int(lib.sx_reinhard_tiles_workspace_bytes(dtype, n, h, w))
                assert size >= last, (dtype, n, h, w)
                assert size >= int(lib.sx_reinhard_workspace_bytes_for(dtype, n, h, w)) >= int(lib.sx_reinhard_workspace_bytes(n, h, w))
                assert size >= int(lib.sx_reinhard_workspace_bytes(n, h, w)) + 6 * 4 * n      # room for the tiles' statistics
                last = size
    for h, w in ((1, 1), (33, 47), (1024, 1024)):
        assert lib.sx_hm_tiles_workspace_bytes(0, h, w) == 0
        last = 0
        for n in (1, 2, 3, 5, 64, 4096):
            size = int(lib.sx_hm_tiles_workspace_bytes(n, h, w))
            assert size >= last and size >= int(lib.sx_hm_workspace_bytes(n, h, w)) + n * 3 * 256 * (4 + 4 + 4 + 1)
            last = size


def test_method_validation_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    mean, std = torch.zeros(4, 3), torch.ones(4, 3)
    norm = Reinhard(device="cuda")
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
        norm.apply(x, ColorStatistics(mean, std))
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
        Reinhard(device="cuda", statistics="tile").transform(x)
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
        HistogramMatching(device="cuda", statistics="tile").transform(x)
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="C=3"):
            norm.estimate(bad)
    # a fitted normaliser (the slots filled by hand: no GPU here), so that the source's shapes are what is refused
    norm._reference_mean, norm._reference_std, norm._is_fitted = torch.zeros(3), torch.ones(3), True
    with pytest.raises(ValueError, match="C=3"):
        norm.apply(torch.zeros(2, 4, 8, 8), (mean, std))
    for src in ((torch.zeros(2, 3), torch.ones(2, 3)), (torch.zeros(4, 2), std), (mean, torch.ones(4, 4)), (torch.zeros(6), torch.ones(3)),
                (mean, torch.ones(1, 3)), (torch.zeros(3), std), (torch.zeros(4, 3, 1), std)):
        with pytest.raises(ValueError, match="shape|rows"):
            norm.apply(x, src)
    with pytest.raises(ValueError, match="source must be"):
        norm.apply(x, mean)
