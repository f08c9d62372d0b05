"""Mask components without a GPU: the three entry points are declared, exported by both libraries and bound with matching arity; every
argument check at the C ABI returns before anything is enqueued (fake pointers that are never dereferenced); the workspace query; the
Python functions validate before any GPU work; and the pin of the GPU tests' yardstick -- on every generator and both connectivities
the union-find restatement of tests/_components_numpy.py IS scipy.ndimage.label, canonicalised, and its filters obey the complement
identity."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import MaskComponents, _native, mask_components, otsu_mask, refine_mask, remove_small_holes, remove_small_objects
from tests import _components_numpy as cn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_mask_components": ("int", 10), "sx_mask_area_filter": ("int", 11), "sx_mask_components_workspace_bytes": ("size_t", 3)}
FAKE, FAKE2, FAKE3, FAKE4 = 1 << 40, 1 << 41, 3 << 40, 5 << 40      # (never dereferenced: every call below fails its checks first)
BAD = _native.SX_ERR_BAD_ARG
PIN_SHAPES = ((520, 200), (33, 47), (5, 4), (1, 130), (130, 1), (1, 1), (64, 64))


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, (restype, params) in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(restype + " " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == params, name
    assert _native.SIGNATURES["sx_mask_components_workspace_bytes"] == _native.SIGNATURES["sx_macenko_workspace_bytes"]
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1
    for name in ("MaskComponents", "mask_components", "remove_small_objects", "remove_small_holes"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.masks, name)
    assert _native.CONNECTIVITIES == stainx_amd.masks.CONNECTIVITIES == cn.CONNECTIVITIES == (4, 8)
    assert MaskComponents._fields == ("labels", "areas", "counts")


def test_components_rejects_bad_arguments_before_any_launch():
    for lib in (_native.require(), _native.require_diag()):
        def call(src=FAKE, n=4, h=64, w=64, connectivity=8, invert=0, labels=FAKE2, areas=FAKE3, counts=FAKE4):
            return lib.sx_mask_components(src, n, h, w, connectivity, invert, labels, areas, counts, None)

        assert call(src=None) == BAD and "mask_in" in _native.last_error(lib)
        assert call(labels=None) == BAD and "labels_out" in _native.last_error(lib)
        for n in (0, -1):
            assert call(n=n) == BAD and "n_tiles" in _native.last_error(lib)
        assert call(h=0) == BAD and "height" in _native.last_error(lib) and call(w=0) == BAD and "width" in _native.last_error(lib)
        assert call(h=-3) == BAD and call(w=-3) == BAD
        for connectivity in (0, 1, 2, 6, 9, -8):
            assert call(connectivity=connectivity) == BAD and "connectivity" in _native.last_error(lib), connectivity
        # a tile of more than 2^31 - 2 pixels has no int32 labels; 2^31 - 2 itself is no argument error of this kind
        assert call(n=1, h=1 << 16, w=1 << 15) == BAD and "2^31 - 2" in _native.last_error(lib)
        assert call(n=1, h=1, w=(1 << 31) - 1) == BAD and "2^31 - 2" in _native.last_error(lib)
        assert call(n=1 << 40, h=64, w=64) == BAD and "too large" in _native.last_error(lib)
        assert call(n=1 << 30, h=1 << 12, w=1 << 12) == BAD and "too large" in _native.last_error(lib)
        assert call(areas=FAKE2) == BAD and "areas_out" in _native.last_error(lib)


def test_area_filter_rejects_bad_arguments_before_any_launch():
    for lib in (_native.require(), _native.require_diag()):
        need = int(lib.sx_mask_components_workspace_bytes(4, 64, 64))

        def call(src=FAKE, out=FAKE2, n=4, h=64, w=64, connectivity=8, holes=0, min_area=16, workspace=FAKE3, counts=None):
            return lib.sx_mask_area_filter(src, out, n, h, w, connectivity, holes, min_area, workspace, counts, None)

        for holes in (0, 1):
            assert call(src=None, holes=holes) == BAD and "mask_in" in _native.last_error(lib)
            assert call(out=None, holes=holes) == BAD and "mask_out" in _native.last_error(lib)
            assert call(workspace=None, holes=holes) == BAD and "workspace" in _native.last_error(lib)
            for n in (0, -1):
                assert call(n=n, holes=holes) == BAD and "n_tiles" in _native.last_error(lib)
            assert call(h=0, holes=holes) == BAD and "height" in _native.last_error(lib) and call(w=-1, holes=holes) == BAD and "width" in _native.last_error(lib)
            for connectivity in (0, 1, 2, 6, 16):
                assert call(connectivity=connectivity, holes=holes) == BAD and "connectivity" in _native.last_error(lib), connectivity
            for min_area in (0, -1, -(1 << 40)):
                assert call(min_area=min_area, holes=holes) == BAD and "min_area" in _native.last_error(lib), min_area
            assert call(n=1, h=1 << 16, w=1 << 15, holes=holes) == BAD and "2^31 - 2" in _native.last_error(lib)
            assert call(n=1 << 40, holes=holes) == BAD and "too large" in _native.last_error(lib)
            assert call(out=FAKE, holes=holes) == BAD and "in place" in _native.last_error(lib)
            # mask_out at the workspace's first byte, in its middle, at its last byte, and ending one byte into it
            for out in (FAKE3, FAKE3 + need // 2, FAKE3 + need - 1, FAKE3 - 4 * 64 * 64 + 1):
                assert call(out=out, holes=holes) == BAD and "workspace" in _native.last_error(lib), out - FAKE3


def test_workspace_query():
    for lib in (_native.require(), _native.require_diag()):
        for sizes in ((0, 64, 64), (4, 0, 64), (4, 64, 0), (-1, 64, 64), (4, -64, 64), (4, 64, -64), (0, 0, 0)):
            assert lib.sx_mask_components_workspace_bytes(*sizes) == 0, sizes
        for n, h, w in ((1, 1, 1), (4, 64, 64), (3, 520, 200), (64, 512, 512), (2, 33, 47)):
            assert 0 < lib.sx_mask_components_workspace_bytes(n, h, w) <= 8 * n * h * w + 4096, (n, h, w)


def test_python_validation_before_gpu_work():
    good = torch.ones(4, 8, 10, dtype=torch.uint8)      # (on the CPU: areas and connectivity are checked first, the mask last)
    bad_masks = [(torch.ones(4, 8, 10, dtype=torch.float32), "dtype"), (torch.ones(4, 8, 10, dtype=torch.int32), "dtype"), (torch.ones(8, 10, dtype=torch.uint8), "shape"),
                 (torch.ones(4, 3, 8, 10, dtype=torch.uint8), "shape"), (good, "device"), (torch.ones(4, 1, 8, 10, dtype=torch.bool), "device"),
                 (np.ones((4, 8, 10), dtype=np.uint8), "tensor")]
    for mask, what in bad_masks:
        with pytest.raises(ValueError, match=what):
            mask_components(mask)
        with pytest.raises(ValueError, match=what):
            mask_components(mask, connectivity=4, holes=True)
        for call in (remove_small_objects, remove_small_holes):
            with pytest.raises(ValueError, match=what):
                call(mask, 5)
        with pytest.raises(ValueError, match=what):
            refine_mask(mask, min_object_area=5, min_hole_area=5, connectivity=4)
    for call in (remove_small_objects, remove_small_holes):
        for min_area in (0, -1, 2.0, "2", None, True, False):
            with pytest.raises(ValueError, match="min_area"):
                call(good, min_area)
        for connectivity in (0, 1, 2, 6, 8.0, "8", None, True):
            with pytest.raises(ValueError, match="connectivity"):
                call(good, 5, connectivity=connectivity)
    for connectivity in (0, 1, 2, 6, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            mask_components(good, connectivity=connectivity)
        with pytest.raises(ValueError, match="connectivity"):
            refine_mask(good, connectivity=connectivity)
        with pytest.raises(ValueError, match="connectivity"):
            otsu_mask(torch.zeros(2, 3, 8, 8), connectivity=connectivity)
    for area in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="min_object_area"):
            refine_mask(good, min_object_area=area)
        with pytest.raises(ValueError, match="min_hole_area"):
            refine_mask(good, min_hole_area=area)
        with pytest.raises(ValueError, match="min_object_area"):
            otsu_mask(torch.zeros(2, 3, 8, 8), min_object_area=area)
        with pytest.raises(ValueError, match="min_hole_area"):
            otsu_mask(torch.zeros(2, 3, 8, 8), min_hole_area=area)
    with pytest.raises(ValueError, match="device"):      # 0 is a valid area there: the mask is what is wrong
        refine_mask(good, min_object_area=0, min_hole_area=0)
    for fn in (remove_small_holes, refine_mask, otsu_mask):      # the hazard is stated where a caller meets it
        assert "glass" in fn.__doc__ and "filled" in fn.__doc__.lower(), fn.__name__


# ------------------------------------------------------------------ the pin of the GPU yardstick
@pytest.mark.parametrize("connectivity", cn.CONNECTIVITIES)
def test_restatement_is_scipy_label_canonicalised(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), dtype=bool)
    for h, w in PIN_SHAPES:
        for name in cn.GENERATORS:
            if (h, w) == (520, 200) and name.startswith("random_") and name not in ("random_0.41", "random_0.593"):
                continue      # (the main shape: the two densities at the thresholds; the others are pinned on the small shapes)
            mask = cn.tile(name, h, w, seed=3)
            for holes in (False, True):
                labels, areas, counts = cn.components(mask[None], connectivity, holes)
                bits = (mask != 0) != holes
                found, n = ndi.label(bits, structure=structure)
                np.testing.assert_array_equal(labels[0], cn.canonical(found), err_msg=f"{name} {h}x{w} holes={holes}")
                assert counts.tolist() == [n] and labels.dtype == np.int32 and areas.dtype == np.int32 and counts.dtype == np.int64
                assert int(areas.sum()) == int(bits.sum())
                np.testing.assert_array_equal(areas[0] != 0, labels[0] == 1 + np.arange(h * w).reshape(h, w))
                sizes = ndi.sum_labels(bits, found, index=np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
                assert sorted(areas[areas != 0].tolist()) == sorted(sizes.tolist())


def test_generators_are_what_they_say():
    h, w = 520, 200
    for connectivity in cn.CONNECTIVITIES:
        assert cn.components(cn.serpentine(h, w)[None], connectivity)[2].tolist() == [1]
        assert cn.components(cn.comb(h, w)[None], connectivity)[2].tolist() == [1]
    assert cn.components(cn.checkerboard(h, w)[None], 4)[2].tolist() == [h * w // 2] and cn.components(cn.checkerboard(h, w)[None], 8)[2].tolist() == [1]
    diag = cn.diagonal(h, w)
    assert diag[255, 63] and diag[256, 64] and diag[255, 64] and diag[256, 63]      # through the corner of the 256 x 64 blocks
    assert cn.components(diag[None], 8)[2].tolist() == [1] and cn.components(diag[None], 4)[2].tolist() == [int(diag.sum()) - 3]
    assert cn.components(cn.frames(h, w)[None], 8)[2].tolist() == [50] and cn.components(cn.frames(h, w)[None], 8, holes=True)[2].tolist() == [50]
    assert int(cn.serpentine(h, w).sum()) == (h // 2) * w + (h // 2 - 1)


@pytest.mark.parametrize("connectivity", cn.CONNECTIVITIES)
def test_filter_restatement_obeys_the_complement_identity(connectivity):
    for h, w in ((33, 47), (5, 4), (1, 130), (1, 1)):
        for name in cn.GENERATORS:
            mask = np.stack([cn.tile(name, h, w, seed=5), cn.tile(name, h, w, seed=6).T.reshape(h, w)])
            for min_area in (1, 2, 5, 40, h * w, h * w + 1):
                objects = cn.remove_small_objects(mask, min_area, connectivity)
                holes = cn.remove_small_holes(mask, min_area, connectivity)
                np.testing.assert_array_equal(holes, 1 - cn.remove_small_objects(1 - mask, min_area, connectivity))
                np.testing.assert_array_equal(objects, 1 - cn.remove_small_holes(1 - mask, min_area, connectivity))
                assert (objects <= mask).all() and (holes >= mask).all()
                if min_area == 1:
                    np.testing.assert_array_equal(objects, mask)
                    np.testing.assert_array_equal(holes, mask)
                if min_area == h * w + 1:
                    assert not objects.any() and holes.all()
