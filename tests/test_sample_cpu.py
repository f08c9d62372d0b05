"""Tissue pixel sampling without a GPU: the rule and the pixel-side test of DESIGN.md 5j, exhaustively over small cases, in Python
integers; the numpy restatement on a case worked by hand; ``PixelSample.cat``; every ValueError of ``sample_pixels``, raised on CPU tensors
before the library is touched; the two entry points declared, exported by both libraries and bound with matching arity; every argument
error at the C ABI, returned before anything is enqueued."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import PixelSample, _native, sample_pixels
from tests import _sample_numpy as sn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_sample_workspace_bytes": 3, "sx_sample_pixels": 17}
FAKE, FAKE2, FAKE3, FAKE4, FAKE5, WS = 1 << 40, 1 << 41, 3 << 40, 5 << 40, 6 << 40, 7 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE


def offsets_for(n: int) -> list[int]:
    return sorted({0, 1, max(n - 1, 0), n, (1 << 40) + 3})


def test_rule_and_pixel_side_test_exhaustively():
    for n in range(0, 41):
        for k in range(1, 13):
            for offset in offsets_for(n):
                ranks = sn.slot_ranks(n, k, offset)
                assert len(ranks) == min(n, k)
                if n <= k:
                    assert ranks == list(range(n)), (n, k, offset)      # the identity, whatever the offset
                    continue
                assert all(b > a for a, b in zip(ranks, ranks[1:])) and 0 <= ranks[0] and ranks[-1] < n, (n, k, offset, ranks)
                # the pixel-side test selects exactly the slots' ranks, each with its slot number
                took = {r: sn.pixel_side(r, n, k, offset) for r in range(n)}
                assert {r: j for r, j in took.items() if j is not None} == {r: j for j, r in enumerate(ranks)}, (n, k, offset)
                # its interval form (what the kernels use): the slots whose rank lies in R0 .. R0 + C - 1 are J(R0) .. J(R0 + C) - 1
                first = [sn.first_slot(r, n, k, offset) for r in range(n + 1)]
                assert first[0] == 0 and first[n] == k and all(b >= a for a, b in zip(first, first[1:])), (n, k, offset)
                for size in (1, 3, 7, n):
                    for begin in range(0, n, size):
                        end = min(begin + size, n)
                        assert [j for j, r in enumerate(ranks) if begin <= r < end] == list(range(first[begin], first[end])), (n, k, offset, begin, end)


def test_restatement_on_a_case_worked_by_hand():
    x = np.arange(2 * 3 * 2 * 4, dtype=np.float32).reshape(2, 3, 2, 4)
    x[0, 1, 0, 1] = -0.0
    mask = np.array([[[0, 2, 0, 1], [255, 0, 1, 1]], [[0, 0, 0, 0], [0, 0, 0, 1]]], dtype=np.uint8)
    # per tile, K = 3: tile 0 has n = 5 (pixels 1, 3, 4, 6, 7), ranks (0, 1, 3) at offset 0 -> pixels 1, 3, 6; tile 1 has n = 1 -> pixel 7 and two empty slots
    pixels, valid, taken, population = sn.sample_pixels(x, (1, 3), mask)
    assert pixels.shape == (2, 3, 1, 3) and pixels.dtype == np.float32 and valid.dtype == np.uint8 and taken.dtype == np.int32 and population.dtype == np.int64
    assert population.tolist() == [5, 1] and taken.tolist() == [3, 1] and valid.reshape(2, 3).tolist() == [[1, 1, 1], [1, 0, 0]]
    assert pixels[0, 0, 0].tolist() == [1.0, 3.0, 6.0] and pixels[0, 2, 0].tolist() == [17.0, 19.0, 22.0]
    assert np.signbit(pixels[0, 1, 0, 0]) and pixels[0, 1, 0, 0] == 0.0                                      # -0.0 keeps its bits
    assert pixels[1, :, 0, 0].tolist() == [31.0, 39.0, 47.0] and not pixels[1, :, 0, 1:].any()
    # offset 2: o = 2, ranks (2 // 3, 7 // 3, 12 // 3) = (0, 2, 4) -> pixels 1, 4, 7
    assert sn.sample_pixels(x, (1, 3), mask, offset=2)[0][0, 0, 0].tolist() == [1.0, 4.0, 7.0]
    # pooled: n = 6, the population is tile 0's five pixels, then tile 1's one; K = 4 -> ranks (0, 1, 3, 4)
    pixels, valid, taken, population = sn.sample_pixels(x, (2, 2), mask, pooled=True)
    assert pixels.shape == (1, 3, 2, 2) and population.tolist() == [6] and taken.tolist() == [4] and valid.all()
    assert pixels[0, 0].reshape(-1).tolist() == [1.0, 3.0, 6.0, 7.0]
    # no mask: every pixel
    assert sn.sample_pixels(x, (1, 8))[0][1, 0, 0].tolist() == x[1, 0].reshape(-1).tolist()


def make_sample(groups: int, h: int, w: int, dtype=torch.float32) -> PixelSample:
    return PixelSample(torch.zeros(groups, 3, h, w, dtype=dtype), torch.ones(groups, h, w, dtype=torch.uint8), torch.full((groups,), h * w, dtype=torch.int32),
                       torch.full((groups,), 1000, dtype=torch.int64))


def test_cat_shapes_and_refusals():
    a, b = make_sample(2, 4, 5), make_sample(1, 4, 5)
    b.pixels.fill_(3.0)
    s = PixelSample.cat(a, b, a)
    assert isinstance(s, PixelSample) and s._fields == ("pixels", "valid", "taken", "population")
    assert s.pixels.shape == (5, 3, 4, 5) and s.valid.shape == (5, 4, 5) and s.taken.shape == (5,) and s.population.shape == (5,)
    assert s.pixels.dtype == torch.float32 and s.valid.dtype == torch.uint8 and s.taken.dtype == torch.int32 and s.population.dtype == torch.int64
    assert torch.equal(s.pixels[2:3], b.pixels) and torch.equal(s.pixels[3:], a.pixels)
    one = PixelSample.cat(b)
    assert torch.equal(one.pixels, b.pixels) and one.pixels.shape == (1, 3, 4, 5)
    with pytest.raises(ValueError, match="at least one"):
        PixelSample.cat()
    with pytest.raises(ValueError, match="same size"):
        PixelSample.cat(a, make_sample(1, 5, 4))
    with pytest.raises(ValueError, match="same element type"):
        PixelSample.cat(a, make_sample(1, 4, 5, torch.uint8))
    with pytest.raises(ValueError, match="expected PixelSamples"):
        PixelSample.cat(a, torch.zeros(1, 3, 4, 5))
    with pytest.raises(ValueError, match="not a PixelSample"):
        PixelSample.cat(PixelSample(a.pixels, a.valid[:1], a.taken, a.population))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="same device"):
            PixelSample.cat(a, PixelSample(*(t.cuda() for t in b)))


def test_value_errors_before_the_library_is_touched(monkeypatch):
    def boom(*args, **kwargs):
        raise AssertionError("the backend must not be reached")

    import stainx_amd.backends.torch_hip_backend as be

    monkeypatch.setattr(be, "sample_pixels_native", boom)
    monkeypatch.setattr(be, "tissue_mask_native", boom)
    x = torch.zeros(2, 3, 8, 9, dtype=torch.uint8)
    for size in (0, -3, (0, 4), (4, 0), (4,), (1, 2, 3), 2.0, (2.0, 2), True, None, "64", (1 << 12, (1 << 12) + 1)):
        with pytest.raises(ValueError, match="size must"):
            sample_pixels(x, size)
    for offset in (-1, 1.0, True, None, 1 << 63):
        with pytest.raises(ValueError, match="offset must"):
            sample_pixels(x, 4, offset=offset)
    for images in (torch.zeros(3, 8, 9), torch.zeros(1, 2, 3, 8, 9), np.zeros((2, 3, 8, 9)), None):
        with pytest.raises(ValueError, match="4-D image tensor"):
            sample_pixels(images, 4)
    with pytest.raises(ValueError, match="3 channels"):
        sample_pixels(torch.zeros(2, 4, 8, 9), 4)
    with pytest.raises(ValueError, match="3 channels"):
        sample_pixels(x, 4, channel_axis=-1)
    with pytest.raises(ValueError, match="Unsupported channel_axis"):
        sample_pixels(x, 4, channel_axis=2)
    with pytest.raises(ValueError, match="unsupported image dtype"):
        sample_pixels(torch.zeros(2, 3, 8, 9, dtype=torch.int32), 4)
    for mask in (torch.ones(2, 9, 8, dtype=torch.uint8), torch.ones(1, 8, 9, dtype=torch.uint8), torch.ones(2, 2, 8, 9, dtype=torch.uint8), torch.ones(8, 9, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask shape must"):
            sample_pixels(x, 4, mask=mask)
    for mask in (torch.ones(2, 8, 9), torch.ones(2, 8, 9, dtype=torch.int64)):
        with pytest.raises(ValueError, match="mask dtype must"):
            sample_pixels(x, 4, mask=mask)
    with pytest.raises(ValueError, match="mask must be"):
        sample_pixels(x, 4, mask=np.ones((2, 8, 9), dtype=np.uint8))
    with pytest.raises(ValueError, match="mask must be None or one of"):
        sample_pixels(x, 4, mask="otsu")
    with pytest.raises(ValueError, match="mask device"):
        sample_pixels(x, 4, mask=torch.ones(2, 8, 9, dtype=torch.uint8))      # (a CPU mask: masks live on the GPU)
    for threshold in (0.0, 1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="luminosity_threshold"):
            sample_pixels(x, 4, mask="luminosity", luminosity_threshold=threshold)
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        sample_pixels(torch.zeros(1, 3, 1, 1, dtype=torch.uint8).expand(1 << 16, 3, 1 << 15, 2), 4, pooled=True)      # (a view: 2^32 pixels, three bytes of storage)


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(r"(?:int|size_t) " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    for name in ("sample_pixels", "PixelSample"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.sampling, name)
    assert PixelSample._fields == ("pixels", "valid", "taken", "population")
    assert stainx_amd.sampling.MAX_SAMPLE_SIZE == _native.MAX_SAMPLE_SIZE == 1 << 24


def test_c_abi_rejects_bad_arguments_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        need = lib.sx_sample_workspace_bytes(4, 64, 64)
        assert need > 0 and need % 256 == 0
        assert lib.sx_sample_workspace_bytes(0, 64, 64) == 0 and lib.sx_sample_workspace_bytes(4, -1, 64) == 0 and lib.sx_sample_workspace_bytes(4, 1 << 16, 1 << 15) == 0
        assert lib.sx_sample_workspace_bytes(64, 512, 512) >= 2 * 4 * 64 * 64      # two words per 4096-pixel chunk

        def call(images=FAKE, dtype=u8, n=4, h=64, w=64, last=0, mask=None, pooled=0, k=16, offset=0, pixels=FAKE2, valid=FAKE3, taken=FAKE4, population=FAKE5, ws=WS, nbytes=need):
            return lib.sx_sample_pixels(images, dtype, n, h, w, last, mask, pooled, k, offset, pixels, valid, taken, population, ws, nbytes, None)

        def said(word):
            return word in _native.last_error(lib)

        assert call(images=None) == BAD and said("images")
        for name in ("pixels", "valid", "taken", "population"):
            assert call(**{name: None}) == BAD and said("output pointer"), name
        assert call(dtype=5) == DTYPE and call(dtype=-1) == DTYPE
        assert call(n=0) == BAD and said("positive") and call(h=0) == BAD and call(w=-2) == BAD      # zero tiles: the caller skips the call, as its neighbours have it
        assert call(k=0) == BAD and said("sample_size") and call(k=-1) == BAD and call(k=(1 << 24) + 1) == BAD and said("2^24")
        assert call(offset=-1) == BAD and said("offset")
        assert call(n=1, h=1 << 16, w=1 << 15, nbytes=1 << 40) == BAD and said("2^31")              # a tile of 2^31 pixels
        assert call(n=2, h=1 << 15, w=1 << 15, pooled=1, nbytes=1 << 40) == BAD and said("pooled")    # two tiles of 2^30 pixels, pooled
        assert call(ws=None) == BAD and said("workspace") and call(nbytes=need - 1) == BAD and said("too small") and call(ws=WS + 4) == BAD and said("aligned")
