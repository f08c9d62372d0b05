"""Saturation-channel tissue detection without a GPU: the entry points are declared, exported by both libraries and bound with matching
arity; the argument checks at the C ABI return before anything is enqueued and the Python functions validate before any GPU work; the
saturation rule is 255 (M - m) / M rounded half up, in exact rationals, for every pair of levels; the numpy median the GPU tests compare
with IS scipy's on every input they use; and otsu_level is pinned to otsu_threshold."""
from __future__ import annotations

import ctypes
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import (LevelHistogram, _native, level_histogram, level_mask, median_filter, otsu_level, otsu_threshold, saturation_map, saturation_mask)
from tests import _saturation_numpy as sn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_saturation_map": 8, "sx_median_filter_u8": 7, "sx_level_histogram": 7, "sx_level_mask_tiles": 8}
NAMES = ("LevelHistogram", "SaturationDetection", "saturation_map", "median_filter", "level_histogram", "otsu_level", "level_mask", "saturation_mask")
FAKE, FAKE2, FAKE3 = 1 << 40, 1 << 41, 3 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.require_diag().sx_version() == 1
    assert f"#define SX_MEDIAN_MAX_SIZE {_native.MEDIAN_MAX_SIZE}\n" in header and _native.MEDIAN_MAX_SIZE == 15
    for name in NAMES:
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.masks, name)
    assert stainx_amd.masks.MEDIAN_SIZES == sn.SIZES == tuple(range(3, _native.MEDIAN_MAX_SIZE + 1, 2))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        def smap(images=FAKE, dtype=u8, n=4, h=64, w=64, last=0, out=FAKE2):
            return lib.sx_saturation_map(images, dtype, n, h, w, last, out, None)

        def med(src=FAKE, out=FAKE2, n=4, h=64, w=64, size=7):
            return lib.sx_median_filter_u8(src, out, n, h, w, size, None)

        def hist(levels=FAKE, n=4, h=64, w=64, pooled=0, counts=FAKE2):
            return lib.sx_level_histogram(levels, n, h, w, pooled, counts, None)

        def lmask(levels=FAKE, n=4, h=64, w=64, cuts=FAKE3, mask=FAKE2, counts=FAKE2 + 4096):
            return lib.sx_level_mask_tiles(levels, n, h, w, cuts, mask, counts, None)

        assert smap(images=None) == BAD and smap(out=None) == BAD
        assert smap(n=0) == BAD and smap(n=-2) == BAD and smap(h=-1) == BAD and smap(w=0) == BAD
        assert smap(dtype=17) == DTYPE and smap(dtype=-1, last=1) == DTYPE
        assert med(src=None) == BAD and med(out=None) == BAD
        assert med(n=0) == BAD and med(n=-1) == BAD and med(h=-3) == BAD and med(w=0) == BAD
        for size in (1, 2, 4, 6, 14, 16, 17, 0, -3, 1 << 20):
            assert med(size=size) == BAD and "size" in _native.last_error(lib), size
        for size in sn.SIZES:
            assert med(size=size, out=FAKE) == BAD and "in place" in _native.last_error(lib), size      # out == in
        assert med(n=1 << 40, h=1 << 20, w=1 << 20) == BAD
        for pooled in (0, 1):
            assert hist(levels=None, pooled=pooled) == BAD and hist(counts=None, pooled=pooled) == BAD
            assert hist(n=0, pooled=pooled) == BAD and hist(n=-2, pooled=pooled) == BAD and hist(h=-1, pooled=pooled) == BAD
        assert lmask(levels=None) == BAD
        assert lmask(mask=None, counts=None) == BAD and "both" in _native.last_error(lib)
        assert lmask(n=0) == BAD and lmask(n=-2) == BAD and lmask(w=-1) == BAD
        assert lmask(cuts=None) == BAD and "tile_thresholds" in _native.last_error(lib)


def test_python_validation_before_gpu_work():
    levels = torch.zeros(4, 8, 10, dtype=torch.uint8)      # (on the CPU: sizes and levels are checked first, the tensor's device last)
    images = torch.zeros(2, 3, 8, 8)
    for size in (1, 2, 4, 16, 17, 0, -3, 7.0, "7", None, True):
        with pytest.raises(ValueError, match="size"):
            median_filter(levels, size)
    for size in (1, 2, 4, 16, 17, -3, 7.0, "7", None, True, False, 0.0, -0.0, "", (), 0j):      # (falsy values that are no int do not skip the median)
        with pytest.raises(ValueError, match="median_size"):
            saturation_mask(images, median_size=size)
    for bad in (255, 256, -1, 8.0, "8", True):
        with pytest.raises(ValueError, match="threshold"):
            saturation_mask(images, threshold=bad)
        with pytest.raises(ValueError, match="fallback"):
            saturation_mask(images, fallback=bad)
        with pytest.raises(ValueError, match="fallback"):
            otsu_level(LevelHistogram(torch.ones(1, 256, dtype=torch.int64), torch.full((1,), 256)), fallback=bad)
    with pytest.raises(ValueError, match="fallback"):
        otsu_level(LevelHistogram(torch.ones(1, 256, dtype=torch.int64), torch.full((1,), 256)), fallback=None)
    bad_levels = [(torch.zeros(4, 8, 10), "dtype"), (torch.zeros(4, 8, 10, dtype=torch.int64), "dtype"), (torch.zeros(8, 10, dtype=torch.uint8), "shape"),
                  (torch.zeros(4, 3, 8, 10, dtype=torch.uint8), "shape"), (levels, "device"), (torch.zeros(4, 1, 8, 10, dtype=torch.bool), "device"),
                  (np.zeros((4, 8, 10), dtype=np.uint8), "tensor")]
    for value, what in bad_levels:
        with pytest.raises(ValueError, match=what):
            median_filter(value, 3)
        with pytest.raises(ValueError, match=what):
            level_histogram(value)
        with pytest.raises(ValueError, match=what):
            level_mask(value, 8)
    for call, name in ((saturation_map, "saturation_map"), (saturation_mask, "saturation_mask")):
        for value in (torch.zeros(3, 8, 8), torch.zeros(2, 4, 8, 8), np.zeros((2, 3, 8, 8))):
            with pytest.raises(ValueError, match=name + " expects"):
                call(value)
        with pytest.raises(ValueError, match=name + " expects"):
            call(images, channel_axis=-1)
        with pytest.raises(ValueError, match="channel_axis"):
            call(images, channel_axis=2)
    for kwargs, what in (({"open_radius": -1}, "open_radius"), ({"close_radius": 32}, "close_radius"), ({"element": "diamond"}, "element"),
                         ({"min_object_area": -1}, "min_object_area"), ({"min_hole_area": 1.5}, "min_hole_area"), ({"connectivity": 6}, "connectivity")):
        with pytest.raises(ValueError, match=what):
            saturation_mask(images, **kwargs)


# ------------------------------------------------------------------ the saturation rule, exactly
def test_saturation_rule_is_the_rounded_quotient_for_every_pair_of_levels():
    hi, lo = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    keep = lo <= hi
    hi, lo = hi[keep], lo[keep]
    got = sn.saturation_of_levels(hi, lo)
    want = [0 if M == 0 else (Fraction(255 * (M - m), M) + Fraction(1, 2)).__floor__() for M, m in zip(hi.tolist(), lo.tolist())]
    np.testing.assert_array_equal(got, np.array(want, dtype=np.int64))
    assert got.min() == 0 and got.max() == 255
    assert (got[lo == 0][1:] == 255).all() and (got[lo == hi] == 0).all()      # a pure colour is 255, a grey 0
    # the hazard the docstring states: near-black pixels have a high saturation
    assert sn.saturation_map(np.array([10, 10, 12], dtype=np.uint8).reshape(1, 3, 1, 1)).item() == 43


def test_levels_of_float_tiles():
    u = torch.arange(256, dtype=torch.uint8)
    for dt in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        lv, nan = sn.levels_of(sn.as_numpy((u.to(torch.float32) / 255.0).to(dt)))
        assert lv.tolist() == list(range(256)) and not nan.any(), dt      # u / 255 has the level u
    # ... in bf16 too, but only just: half a unit in the last of its 8 bits moves 255 v by up to 255 * 2^-9 = 0.498 of a level
    assert 255 * 2.0 ** -9 < 0.5
    worst = (np.float32(255) * sn.as_numpy((u.float() / 255.0).to(torch.bfloat16)).astype(np.float32) - np.arange(256)).__abs__().max()
    assert 0.4 < worst < 0.5
    lv, nan = sn.levels_of(np.array([-0.5, -np.inf, np.inf, 1.5, np.nan, 0.0, 1.0, 0.3, 0.25, 0.75], dtype=np.float32))
    assert lv.tolist() == [0, 0, 255, 255, 0, 0, 255, 76, 64, 191] and nan.tolist() == [False] * 4 + [True] + [False] * 5      # 63.75 -> 64, 191.25 -> 191


# ------------------------------------------------------------------ the median restatement IS scipy's
@pytest.mark.parametrize("size", sn.SIZES)
def test_numpy_median_is_scipy(size):
    import scipy.ndimage as ndi      # (a plain import: without scipy this test FAILS -- it is the one independent check of the restatement the GPU tests compare with)

    for name in sn.GENERATORS:
        levels = sn.levels_case(name)
        want = np.stack([ndi.median_filter(tile, size=size, mode="nearest") for tile in levels])
        np.testing.assert_array_equal(sn.median_case(name, size), want, err_msg=f"{name} {size}")
        if name == "mask01":
            np.testing.assert_array_equal(sn.majority(levels, size), want, err_msg=f"majority {size}")
    if size in (3, 15):
        for shape in sn.SMALL_SHAPES:
            levels = sn.levels_case("random", shape)
            want = np.stack([ndi.median_filter(tile, size=size, mode="nearest") for tile in levels])
            np.testing.assert_array_equal(sn.median_case("random", size, shape), want, err_msg=f"{shape} {size}")


def test_numpy_median_complement_identity():
    levels = sn.levels_case("random", (2, 2, 5))
    for size in (3, 15):
        np.testing.assert_array_equal(sn.median(255 - levels, size), 255 - sn.median(levels, size))


# ------------------------------------------------------------------ otsu_level and pool
def as_hist(rows) -> LevelHistogram:
    counts = torch.tensor(rows, dtype=torch.int64).reshape(-1, 256)
    return LevelHistogram(counts, counts.sum(dim=1))


def test_otsu_level_is_pinned_to_otsu_threshold():
    rng = np.random.default_rng(5)
    rows = [rng.integers(0, 1000, 256).tolist() for _ in range(6)]
    rows += [(rng.integers(0, 50, 256) * (rng.random(256) < 0.1)).tolist() for _ in range(6)]
    rows.append([0] * 256)
    for fallback in (0, 8, 254):
        got = otsu_level(as_hist(rows), fallback=fallback)
        assert got.dtype == torch.int64 and got.device.type == "cpu" and got.shape == (len(rows),)
        cut = otsu_threshold(as_hist(rows), fallback=(fallback + 1) / 256)
        assert got.tolist() == [int(k) - 1 for k in (cut * 256).tolist()] and all(float(k).is_integer() for k in (cut * 256).tolist())
        assert 0 <= min(got.tolist()) and max(got.tolist()) <= 254 and got[-1].item() == fallback
    assert otsu_level(as_hist(rows)).tolist() == otsu_level(as_hist(rows), fallback=8).tolist()      # CLAM's 8 is the default


def test_otsu_level_two_modes_take_the_middle_of_the_gap():
    for a, b, ca, cb in ((10, 200, 5, 7), (0, 255, 1, 1), (100, 101, 3, 9), (40, 43, 10 ** 6, 1)):
        row = [0] * 256
        row[a], row[b] = ca, cb
        t = otsu_level(as_hist([row])).item()
        assert t == (a + 1 + b) // 2 - 1 and a <= t < b, (a, b)      # background = levels <= t: every t in a..b-1 splits the spikes
    row = [0] * 256
    row[20:31] = [5] * 11
    row[180:201] = [9] * 21
    t = otsu_level(as_hist([row])).item()
    assert t == (31 + 180) // 2 - 1      # modes 20..30 and 180..200: t in 30..179 splits them, the middle it is


def test_otsu_level_one_bin_or_none_is_the_fallback():
    for bin_ in (0, 17, 255):
        row = [0] * 256
        row[bin_] = 12345
        assert otsu_level(as_hist([row])).item() == 8 and otsu_level(as_hist([row]), fallback=0).item() == 0
        assert otsu_level(as_hist([row]), fallback=254).item() == 254 and otsu_level(as_hist([row]), fallback=100).item() == 100
    assert otsu_level(as_hist([[0] * 256]), fallback=61).item() == 61


def test_level_histogram_pool_adds_exactly():
    rng = np.random.default_rng(3)
    a = as_hist(rng.integers(0, 1 << 40, (3, 256)).tolist())
    b = as_hist(rng.integers(0, 1 << 40, (1, 256)).tolist())
    pooled = LevelHistogram.pool(a, b)
    assert isinstance(pooled, LevelHistogram) and pooled.counts.shape == (1, 256) and pooled.pixels.shape == (1,)
    want = [sum(int(a.counts[i, k]) for i in range(3)) + int(b.counts[0, k]) for k in range(256)]
    assert pooled.counts[0].tolist() == want and int(pooled.pixels[0]) == sum(want)
    assert torch.equal(LevelHistogram.pool(b).counts, b.counts)
    with pytest.raises(ValueError, match="at least one"):
        LevelHistogram.pool()
    for bad, what in (((a.counts[:, :255], a.pixels), "shape"), ((a.counts, a.pixels[:2]), "shape"), ((a.counts.float(), a.pixels), "dtype")):
        with pytest.raises(ValueError, match=what):
            LevelHistogram.pool(a, bad)
