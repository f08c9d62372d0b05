"""Slide-level histogram matching without a GPU: the new entry points are exported by both libraries and declared, their argument checks
at the C ABI return before anything is enqueued, the class validates before any GPU work, and ``HistogramStatistics.pool`` adds exactly."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest
import torch

import stainx_amd
from stainx_amd import HistogramMatching, HistogramStatistics, _native

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_hm_estimate": 12, "sx_hm_estimate_masked": 14, "sx_hm_tables": 6, "sx_hm_apply_tables": 10, "sx_hm_apply_tables_masked": 12}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(r"int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1
    assert _native.require_diag().sx_version() == 1


def test_public_names():
    assert "HistogramStatistics" in stainx_amd.__all__
    assert stainx_amd.HistogramStatistics is HistogramStatistics
    assert HistogramStatistics._fields == ("counts", "pixels")
    for name in ("estimate", "lookup_tables", "apply"):
        assert callable(getattr(HistogramMatching, name))


@pytest.mark.parametrize("which", ["product", "diag"])
def test_estimate_rejects_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    u8 = _native.DTYPE_CODES[torch.uint8]
    need = int(lib.sx_hm_tiles_workspace_bytes(4, 64, 64))
    need_masked = int(lib.sx_hm_masked_workspace_bytes(4, 64, 64))

    def est(images=FAKE, dtype=u8, n=4, last=0, per_tile=1, counts=FAKE, pixels=FAKE, ws=FAKE, nbytes=need):
        return lib.sx_hm_estimate(images, dtype, n, 64, 64, last, per_tile, counts, pixels, ws, nbytes, None)

    def est_masked(images=FAKE, dtype=u8, n=4, last=0, per_tile=1, mask=FAKE, threshold=0.8, counts=FAKE, pixels=FAKE, ws=FAKE, nbytes=need_masked):
        return lib.sx_hm_estimate_masked(images, dtype, n, 64, 64, last, per_tile, mask, threshold, counts, pixels, ws, nbytes, None)

    for call in (est, est_masked):
        assert call(images=None) == BAD
        assert call(counts=None) == BAD
        assert call(n=0) == BAD and call(n=-1) == BAD
        assert call(dtype=17) == DTYPE
        assert call(dtype=-1, per_tile=0, last=1) == DTYPE
        assert call(ws=None) == WORKSPACE
        assert call(ws=FAKE + 8) == WORKSPACE
        assert call(nbytes=int(lib.sx_hm_workspace_bytes(4, 64, 64))) == WORKSPACE      # (the pooled size does not do, for a pooled call either)
        assert call(nbytes=int(lib.sx_hm_workspace_bytes(4, 64, 64)), per_tile=0) == WORKSPACE
    assert est(nbytes=need - 1) == WORKSPACE
    assert est_masked(nbytes=need_masked - 1) == WORKSPACE
    for threshold in (0.0, 1.0, -0.5, 1.5, float("nan")):      # the rule (no mask) needs a threshold inside (0, 1)
        assert est_masked(mask=None, threshold=threshold) == BAD and "luminosity_threshold" in _native.last_error(lib), threshold
    assert est_masked(mask=FAKE, threshold=7.0, nbytes=0) == WORKSPACE      # (not read when a mask is given: the next check answers)


@pytest.mark.parametrize("which", ["product", "diag"])
def test_tables_rejects_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()

    def call(counts=FAKE, pixels=FAKE, n_sets=4, ref=FAKE, lut=FAKE):
        return lib.sx_hm_tables(counts, pixels, n_sets, ref, lut, None)

    assert call(counts=None) == BAD
    assert call(pixels=None) == BAD      # (device memory, required: there is no host-side pixel total)
    assert call(ref=None) == BAD
    assert call(lut=None) == BAD
    assert call(n_sets=0) == BAD and call(n_sets=-2) == BAD
    assert call(n_sets=1 << 40) == BAD


@pytest.mark.parametrize("which", ["product", "diag"])
def test_apply_tables_rejects_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32 = _native.DTYPE_CODES[torch.float32]

    def plain(images=FAKE, out=FAKE, dtype=f32, n=4, last=0, lut=FAKE, n_sources=4):
        return lib.sx_hm_apply_tables(images, out, dtype, n, 64, 64, last, lut, n_sources, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=4, last=0, lut=FAKE, n_sources=4, mask=FAKE, threshold=0.8):
        return lib.sx_hm_apply_tables_masked(images, out, dtype, n, 64, 64, last, lut, n_sources, mask, threshold, None)

    for call in (plain, masked):
        assert call(images=None) == BAD
        assert call(out=None) == BAD
        assert call(lut=None) == BAD
        assert call(n=0) == BAD and call(n=-1) == BAD
        for n_sources in (0, 2, 3, 5, -1):      # n = 4: neither 1 nor n
            assert call(n_sources=n_sources) == BAD and "n_sources" in _native.last_error(lib), n_sources
        assert call(dtype=17) == DTYPE
        assert call(dtype=17, n_sources=1, last=1) == DTYPE
    for threshold in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert masked(mask=None, threshold=threshold) == BAD and "luminosity_threshold" in _native.last_error(lib), threshold
    assert masked(mask=FAKE, threshold=7.0, dtype=17) == DTYPE      # (not read when a mask is given)


def test_method_validation_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    tables = torch.zeros(4, 3, 256)
    stats = HistogramStatistics(torch.zeros(4, 3, 256, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    norm = HistogramMatching(device="cuda")
    for source in (tables, stats):
        with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
            norm.apply(x, source)
    with pytest.raises(ValueError, match=r"Must call fit\(\) before transform\(\)"):
        norm.lookup_tables(stats)
    # 3 channels on the configured axis, for the three methods that take images
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8), torch.zeros(2, 8, 8, 3)):
        with pytest.raises(ValueError, match="3 channels on axis 1"):
            norm.estimate(bad)
    last = HistogramMatching(device="cuda", channel_axis=-1)
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(8, 8, 3)):
        with pytest.raises(ValueError, match="3 channels on axis -1"):
            last.estimate(bad)
    # a fitted normaliser (the slots filled by hand: no GPU here), so that the source's shapes are what is refused
    hist = torch.full((256,), 1.0 / 256)
    norm._ref_histograms_256, norm._reference_histogram, norm._is_fitted = [hist, hist, hist], hist, True
    with pytest.raises(ValueError, match="3 channels on axis 1"):
        norm.apply(torch.zeros(2, 4, 8, 8), tables)
    for source in (torch.zeros(2, 3, 256), torch.zeros(5, 3, 256), torch.zeros(4, 3, 255), torch.zeros(4, 2, 256), torch.zeros(256), torch.zeros(1, 4, 3, 256),
                   torch.zeros(0, 3, 256)):
        with pytest.raises(ValueError, match="shape"):
            norm.apply(x, source)
    for source in (tables.double(), tables.half(), torch.zeros(4, 3, 256, dtype=torch.int64)):
        with pytest.raises(ValueError, match="dtype float32"):
            norm.apply(x, source)
    counts, pixels = stats
    for source in (HistogramStatistics(counts[:2], pixels[:2]), (counts, pixels[:3]), (counts[:, :2], pixels), (counts[0], pixels), (counts, pixels.reshape(4, 1))):
        with pytest.raises(ValueError, match="shape|rows"):
            norm.apply(x, source)
    for source in ((counts.int(), pixels), (counts, pixels.int()), (counts.float(), pixels)):
        with pytest.raises(ValueError, match="int64"):
            norm.apply(x, source)
        with pytest.raises(ValueError, match="int64"):
            norm.lookup_tables(source)
    for source in (None, "tile", (counts, pixels, pixels), [counts.numpy(), pixels.numpy()]):
        with pytest.raises(ValueError, match="source must be"):
            norm.apply(x, source)
    with pytest.raises(ValueError, match="source must be"):
        norm.lookup_tables(tables)
    with pytest.raises(ValueError, match="mask"):      # an explicit mask is checked against the images first as well
        norm.apply(x, tables, mask=torch.zeros(4, 9, 8, dtype=torch.uint8))


def test_pool_adds_exactly_in_int64():
    big = (1 << 32) + 12345      # more than a 32-bit counter, or a float32, can hold exactly
    g = torch.Generator().manual_seed(5)
    a = HistogramStatistics(torch.randint(0, 1 << 20, (3, 3, 256), generator=g) + big, torch.tensor([big * 256 + 1, 7, 0]))
    b = HistogramStatistics(torch.randint(0, 1 << 20, (1, 3, 256), generator=g) + 3 * big, torch.tensor([(1 << 45) + 3]))
    c = HistogramStatistics(torch.zeros((2, 3, 256), dtype=torch.int64), torch.zeros((2,), dtype=torch.int64))
    pooled = HistogramStatistics.pool(a, b, c)
    assert isinstance(pooled, HistogramStatistics)
    assert pooled.counts.dtype == torch.int64 and pooled.pixels.dtype == torch.int64
    assert tuple(pooled.counts.shape) == (1, 3, 256) and tuple(pooled.pixels.shape) == (1,)
    want = [[sum(int(s.counts[k, ch, bin_]) for s in (a, b, c) for k in range(s.counts.shape[0])) for bin_ in range(256)] for ch in range(3)]
    assert pooled.counts[0].tolist() == want      # (Python integers: no rounding anywhere)
    assert min(min(row) for row in want) > 6 * (1 << 32)
    assert int(pooled.pixels[0]) == big * 256 + 1 + 7 + (1 << 45) + 3
    # one argument: its sets summed; pooling is associative
    alone = HistogramStatistics.pool(a)
    assert torch.equal(alone.counts[0], a.counts.sum(0)) and int(alone.pixels[0]) == big * 256 + 8
    again = HistogramStatistics.pool(HistogramStatistics.pool(a, b), c)
    assert torch.equal(again.counts, pooled.counts) and torch.equal(again.pixels, pooled.pixels)
    with pytest.raises(ValueError, match="at least one"):
        HistogramStatistics.pool()
    with pytest.raises(ValueError, match="int64"):
        HistogramStatistics.pool(a, HistogramStatistics(b.counts.int(), b.pixels))
