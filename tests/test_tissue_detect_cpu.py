"""Tissue detection without a GPU: the entry points are declared, exported by both libraries and bound with matching arity; their argument
checks at the C ABI return before anything is enqueued; the Python functions validate before any GPU work; Otsu's threshold is pinned,
exactly, to its restatement in rational arithmetic; and the pins of the GPU tests' yardsticks -- the numpy morphology IS scipy's, and
no cut of the 255 has more than a hundredth of an input's pixels within the band in which the oracle does not decide."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import LuminosityHistogram, _native, luminosity_histogram, mask_morphology, otsu_mask, otsu_threshold, refine_mask
from tests import _tissue_detect_numpy as td
from tests.test_tissue_mask_cpu import BAD_THRESHOLDS

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_luminosity_histogram": 9, "sx_tissue_mask_tiles": 10, "sx_mask_morphology": 11}
FAKE, FAKE2, FAKE3 = 1 << 40, 1 << 41, 3 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for names, restype in ((CALLS, "int"), ({"sx_tissue_y_cut": 1}, "float")):
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
    assert f"#define SX_MORPH_MAX_RADIUS {_native.MORPH_MAX_RADIUS}\n" in header and _native.MORPH_MAX_RADIUS >= 15
    for name, code in list(_native.MORPH_OPS.items()) + list(_native.MORPH_ELEMENTS.items()):
        prefix = "SX_ELEMENT_" if name in _native.MORPH_ELEMENTS else "SX_MORPH_"
        assert f"#define {prefix}{name.upper()} {code}\n" in header
    for name in ("LuminosityHistogram", "TissueDetection", "luminosity_histogram", "otsu_threshold", "otsu_mask", "mask_morphology", "refine_mask"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.masks, name)
    assert stainx_amd.masks.MASK_MODES == ("luminosity",) and stainx_amd.masks.MAX_MORPHOLOGY_RADIUS == _native.MORPH_MAX_RADIUS == td.MAX_RADIUS


def test_histogram_and_tile_cuts_reject_bad_arguments_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        def hist(images=FAKE, dtype=u8, n=4, last=0, pooled=0, counts=FAKE):
            return lib.sx_luminosity_histogram(images, dtype, n, 64, 64, last, pooled, counts, None)

        def tiles(images=FAKE, dtype=u8, n=4, last=0, cuts=FAKE, mask=FAKE, counts=FAKE):
            return lib.sx_tissue_mask_tiles(images, dtype, n, 64, 64, last, cuts, mask, counts, None)

        for pooled in (0, 1):
            assert hist(images=None, pooled=pooled) == BAD and hist(counts=None, pooled=pooled) == BAD
            assert hist(n=0, pooled=pooled) == BAD and hist(n=-2, pooled=pooled) == BAD
            assert hist(dtype=17, pooled=pooled) == DTYPE and hist(dtype=-1, last=1, pooled=pooled) == DTYPE
        assert tiles(images=None) == BAD
        assert tiles(mask=None, counts=None) == BAD and "both" in _native.last_error(lib)
        assert tiles(n=0) == BAD and tiles(n=-2) == BAD
        assert tiles(cuts=None) == BAD and "tile_y_cut" in _native.last_error(lib)
        assert tiles(dtype=17) == DTYPE and tiles(dtype=-1, last=1) == DTYPE


def test_morphology_rejects_bad_arguments_before_any_launch():
    top = _native.MORPH_MAX_RADIUS
    for lib in (_native.require(), _native.require_diag()):
        def call(src=FAKE, out=FAKE2, n=4, h=64, w=64, op=0, element=1, radius=2, scratch=None, counts=None):
            return lib.sx_mask_morphology(src, out, n, h, w, op, element, radius, scratch, counts, None)

        assert call(src=None) == BAD and call(out=None) == BAD
        assert call(n=0) == BAD and call(n=-1) == BAD and call(h=0) == BAD and call(w=0) == BAD
        for radius in (0, -1, top + 1, 1 << 20):
            assert call(radius=radius) == BAD and "radius" in _native.last_error(lib), radius
        for op in (-1, 4, 17):
            assert call(op=op) == BAD and "op" in _native.last_error(lib), op
        for element in (-1, 2, 9):
            assert call(element=element) == BAD and "element" in _native.last_error(lib), element
        for op in range(4):
            assert call(op=op, out=FAKE, scratch=FAKE3) == BAD and "in place" in _native.last_error(lib), op      # in place
        for op in (2, 3):
            assert call(op=op) == BAD and "scratch" in _native.last_error(lib), op      # open / close without scratch
            assert call(op=op, scratch=FAKE) == BAD and call(op=op, scratch=FAKE2) == BAD
        assert call(n=1 << 40, h=1 << 20, w=1 << 20) == BAD


def test_tissue_y_cut():
    for lib in (_native.require(), _native.require_diag()):
        for bad in BAD_THRESHOLDS:
            assert math.isnan(lib.sx_tissue_y_cut(bad)), bad
        cuts = [lib.sx_tissue_y_cut(k / 256.0) for k in range(1, 256)]
        assert all(math.isfinite(c) and c > 0.0 for c in cuts)
        assert all(a < b for a, b in zip(cuts, cuts[1:]))      # strictly increasing: the bin rule's search relies on it
        assert np.float32(cuts[0]) == np.float32(cuts[0]) and cuts[-1] < 1.0
    # the constant of the default threshold: L* = 80 -> f = 96 / 116 -> Y = f^3
    assert _native.require().sx_tissue_y_cut(0.8) == float(np.float32((96.0 / 116.0) ** 3))


def test_python_validation_before_gpu_work():
    good = torch.ones(4, 8, 10, dtype=torch.uint8)      # (on the CPU: names and radii are checked first, the mask last)
    bad_masks = [(torch.ones(4, 8, 10, dtype=torch.float32), "dtype"), (torch.ones(4, 8, 10, dtype=torch.int64), "dtype"),
                 (torch.ones(8, 10, dtype=torch.uint8), "shape"), (torch.ones(4, 3, 8, 10, dtype=torch.uint8), "shape"),
                 (torch.ones(4, 8, 10, 1, 1, dtype=torch.bool), "shape"), (torch.ones(4, 8, 10, dtype=torch.uint8), "device"),
                 (torch.ones(4, 1, 8, 10, dtype=torch.bool), "device"), (np.ones((4, 8, 10), dtype=np.uint8), "tensor")]
    for mask, what in bad_masks:
        with pytest.raises(ValueError, match=what):
            mask_morphology(mask, "open", 2)
        with pytest.raises(ValueError, match=what):
            refine_mask(mask, open_radius=2)
    for radius in (0, -1, td.MAX_RADIUS + 1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="radius"):
            mask_morphology(good, "erode", radius)
    for radius in (-1, td.MAX_RADIUS + 1, 1.5, None):
        with pytest.raises(ValueError, match="open_radius"):
            refine_mask(good, open_radius=radius)
        with pytest.raises(ValueError, match="close_radius"):
            refine_mask(good, close_radius=radius)
        with pytest.raises(ValueError, match="close_radius"):
            otsu_mask(torch.zeros(2, 3, 8, 8), close_radius=radius)
    for op in ("opening", "", None, 2):
        with pytest.raises(ValueError, match="op must be"):
            mask_morphology(good, op, 2)
    for element in ("diamond", "", None, 1):
        with pytest.raises(ValueError, match="element"):
            mask_morphology(good, "open", 2, element=element)
        with pytest.raises(ValueError, match="element"):
            refine_mask(good, open_radius=1, element=element)
        with pytest.raises(ValueError, match="element"):
            otsu_mask(torch.zeros(2, 3, 8, 8), element=element)
    for call, name in ((luminosity_histogram, "luminosity_histogram"), (otsu_mask, "otsu_mask")):
        for images in (torch.zeros(3, 8, 8), torch.zeros(2, 4, 8, 8), np.zeros((2, 3, 8, 8))):
            with pytest.raises(ValueError, match=name + " expects"):
                call(images)
        with pytest.raises(ValueError, match=name + " expects"):
            call(torch.zeros(2, 3, 8, 8), channel_axis=-1)
        with pytest.raises(ValueError, match="channel_axis"):
            call(torch.zeros(2, 3, 8, 8), channel_axis=2)
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="luminosity_threshold"):
            otsu_mask(torch.zeros(2, 3, 8, 8), fallback=bad)
        with pytest.raises(ValueError, match="luminosity_threshold"):
            otsu_threshold(LuminosityHistogram(torch.ones(1, 256, dtype=torch.int64), torch.full((1,), 256)), fallback=bad)
    with pytest.raises(ValueError, match="device"):
        mask_morphology(good, "close", td.MAX_RADIUS, element="square")
    # mask="otsu" is no constructor mode
    with pytest.raises(ValueError, match="mask"):
        stainx_amd.Reinhard(device="cuda", mask="otsu")


# ------------------------------------------------------------------ Otsu, exactly
def as_hist(rows) -> LuminosityHistogram:
    counts = torch.tensor(rows, dtype=torch.int64).reshape(-1, 256)
    return LuminosityHistogram(counts, counts.sum(dim=1))


def check_rows(rows, fallback=0.8):
    got = otsu_threshold(as_hist(rows), fallback=fallback)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (len(rows),)
    want = td.otsu_thresholds(np.array(rows, dtype=object), fallback)
    np.testing.assert_array_equal(got.numpy(), want)
    return got.numpy() * 256.0


def test_otsu_is_its_exact_restatement():
    rng = np.random.default_rng(5)
    rows = [rng.integers(0, 1000, 256).tolist() for _ in range(6)]
    rows += [(rng.integers(0, 50, 256) * (rng.random(256) < 0.1)).tolist() for _ in range(6)]      # sparse
    bimodal = np.zeros(256, dtype=np.int64)
    bimodal += np.bincount(np.clip(rng.normal(90, 12, 20000), 0, 255).astype(int), minlength=256)
    bimodal += np.bincount(np.clip(rng.normal(235, 5, 30000), 0, 255).astype(int), minlength=256)
    rows.append(bimodal.tolist())
    ks = check_rows(rows)
    assert ((ks >= 1) & (ks <= 255) & (ks == np.round(ks))).all()      # on the k / 256 lattice
    assert 120 <= ks[-1] <= 225      # between the two modes


def test_otsu_two_spikes_take_the_middle_of_the_gap():
    for a, b, ca, cb in ((10, 200, 5, 7), (0, 255, 1, 1), (100, 101, 3, 9), (40, 43, 10 ** 6, 1)):
        row = [0] * 256
        row[a], row[b] = ca, cb
        assert check_rows([row])[0] == (a + 1 + b) // 2, (a, b)      # every k in a+1..b splits the spikes


def test_otsu_one_populated_bin_or_none_is_the_fallback():
    for bin_ in (0, 17, 255):
        row = [0] * 256
        row[bin_] = 12345
        assert check_rows([row], fallback=0.8)[0] == 0.8 * 256 and check_rows([row], fallback=0.37)[0] == 0.37 * 256
    assert check_rows([[0] * 256], fallback=0.61)[0] == 0.61 * 256


def test_otsu_maximisers_that_are_not_contiguous():
    row = [0] * 256
    row[10], row[19], row[21], row[30] = 1, 4, 4, 1      # symmetric: cutting off either outer spike beats cutting through the middle
    assert td.otsu_maximisers(row) == list(range(11, 20)) + list(range(22, 31))
    assert check_rows([row])[0] == (11 + 30) // 2 == 20      # (no maximiser itself: the rule is the middle of first and last)
    # three equal spikes: one plateau from the first gap to the second
    row = [0] * 256
    row[10] = row[20] = row[30] = 4
    assert td.otsu_maximisers(row) == list(range(11, 31)) and check_rows([row])[0] == 20
    # an asymmetric row for contrast: one gap wins
    row = [0] * 256
    row[10], row[19], row[21], row[30] = 2, 4, 4, 1
    assert td.otsu_maximisers(row) == list(range(11, 20)) and check_rows([row])[0] == 15


def test_otsu_counts_near_two_to_the_forty():
    rng = np.random.default_rng(9)
    rows = [(rng.integers(0, 1 << 40, 256) + (1 << 40)).tolist() for _ in range(3)]
    two = [0] * 256
    two[3], two[250] = (1 << 40) + 1, (1 << 40) - 1
    rows.append(two)
    nearly = [1 << 40] * 256
    nearly[128] += 1      # a float64 could not tell these maxima apart
    rows.append(nearly)
    ks = check_rows(rows)
    assert ks[3] == (4 + 250) // 2


def test_pool_adds_exactly_and_refuses_mismatched_shapes():
    rng = np.random.default_rng(3)
    a = as_hist(rng.integers(0, 1 << 40, (3, 256)).tolist())
    b = as_hist(rng.integers(0, 1 << 40, (1, 256)).tolist())
    pooled = LuminosityHistogram.pool(a, b)
    assert isinstance(pooled, LuminosityHistogram) and pooled.counts.shape == (1, 256) and pooled.pixels.shape == (1,)
    want = [sum(int(a.counts[i, k]) for i in range(3)) + int(b.counts[0, k]) for k in range(256)]
    assert pooled.counts[0].tolist() == want and int(pooled.pixels[0]) == sum(want)
    assert torch.equal(LuminosityHistogram.pool(b).counts, b.counts)
    with pytest.raises(ValueError, match="at least one"):
        LuminosityHistogram.pool()
    for bad, what in (((a.counts[:, :255], a.pixels), "shape"), ((a.counts, a.pixels[:2]), "shape"), ((a.counts.reshape(3, 1, 256), a.pixels), "shape"),
                      ((a.counts.float(), a.pixels), "dtype"), ((a.counts, a.pixels.int()), "dtype"), ((a.counts,), "LuminosityHistogram"), (a.counts, "LuminosityHistogram")):
        with pytest.raises(ValueError, match=what):
            LuminosityHistogram.pool(a, bad)
        if not isinstance(bad, torch.Tensor):
            with pytest.raises(ValueError, match=what):
                otsu_threshold(bad)


# ------------------------------------------------------------------ the pins of the GPU yardsticks
@pytest.mark.parametrize("element", td.ELEMENTS)
def test_numpy_morphology_is_scipy(element):
    ndi = pytest.importorskip("scipy.ndimage")
    for shape, seed in (((2, 7, 5), 1), ((2, 37, 70), 2), ((3, 3, 4), 3)):      # (the last: smaller than every element)
        for density in (0.3, 0.9):
            mask = td.random_mask(shape, density, seed)
            for radius in (1, 2, 5, 15, td.MAX_RADIUS):
                fp = td.footprint(radius, element)
                assert fp.shape == (2 * radius + 1,) * 2 and fp[radius].all() and fp[:, radius].all()
                if element == "disk":
                    assert [int(row.sum()) for row in fp[radius:]] == [2 * hw + 1 for hw in td.half_widths(radius, element)]
                eroded = np.stack([ndi.binary_erosion(m != 0, structure=fp, border_value=1) for m in mask])
                dilated = np.stack([ndi.binary_dilation(m != 0, structure=fp, border_value=0) for m in mask])
                np.testing.assert_array_equal(td.morphology(mask, "erode", radius, element), eroded, err_msg=f"{shape} {radius}")
                np.testing.assert_array_equal(td.morphology(mask, "dilate", radius, element), dilated, err_msg=f"{shape} {radius}")
                opened = np.stack([ndi.binary_dilation(m, structure=fp, border_value=0) for m in eroded])
                closed = np.stack([ndi.binary_erosion(m, structure=fp, border_value=1) for m in dilated])
                np.testing.assert_array_equal(td.morphology(mask, "open", radius, element), opened, err_msg=f"{shape} {radius}")
                np.testing.assert_array_equal(td.morphology(mask, "close", radius, element), closed, err_msg=f"{shape} {radius}")
    # tissue that touches the edge is not eaten from the edge; 255 is set
    full = np.full((1, 6, 9), 255, dtype=np.uint8)
    for op in td.OPS:
        assert td.morphology(full, op, 2, element).all() and not td.morphology(np.zeros_like(full), op, 2, element).any()


@pytest.mark.parametrize("dtype_name", ["u8", "f32", "bf16"])
def test_few_pixels_lie_near_any_one_cut(dtype_name):
    for case in td.ORACLE_CASES:
        below, near = td.oracle_histogram(case, dtype_name)
        pixels = td.tiles_u8(case)[0, 0].numel() * td.tiles_u8(case).shape[0]
        assert below.shape == near.shape == (td.tiles_u8(case).shape[0], 255) and (np.diff(below, axis=1) >= 0).all() and below.max() <= pixels
        share = near.sum(axis=0).max() / pixels
        print(f"{case} {dtype_name}: worst share of pixels within {td.L_BAND} of one cut {share:.2e}")
        assert share <= td.BAND_CAP, (case, dtype_name, share)
