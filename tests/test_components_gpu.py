"""Mask components on the GPU, every result an integer and every check exact: labels, areas and counts against the union-find
restatement of tests/_components_numpy.py (pinned to scipy.ndimage.label in the CPU tests) on every generator, both connectivities,
objects and holes; tile independence; the area filters at the areas where a component is just kept and just removed; the input forms
mask_morphology takes; refine_mask / otsu_mask with and without the new arguments; real tissue; the raw C ABI with its NULL-able
outputs NULL; and a captured graph that reads the mask at replay.

Shapes: (3, 520, 200) is three row blocks by four column blocks of the kernels' 256 x 64 block, with a ragged last block both ways;
(2, 64, 64) is exactly one block wide (and takes the path without a seam launch, as every shape of one block does)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import MaskComponents, _native, mask_components, mask_morphology, otsu_mask, refine_mask, remove_small_holes, remove_small_objects
from tests import _components_numpy as cn
from tests import _tissue_detect_numpy as td

pytestmark = pytest.mark.gpu

MAIN = (3, 520, 200)
SMALL = ((2, 33, 47), (1, 5, 4), (4, 1, 130), (4, 130, 1), (1, 1, 1), (2, 64, 64))
FORMS = [(connectivity, holes) for connectivity in cn.CONNECTIVITIES for holes in (False, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def on(dev, mask: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(mask)).to(dev)      # (a copy: the shared batches are read-only)


def assert_components(got: MaskComponents, want, mask: np.ndarray, holes: bool, what) -> None:
    labels, areas, counts = want
    assert isinstance(got, MaskComponents) and got.labels.dtype == torch.int32 and got.areas.dtype == torch.int32 and got.counts.dtype == torch.int64, what
    assert got.labels.shape == got.areas.shape == mask.shape and got.counts.shape == (mask.shape[0],), what
    got_labels, got_areas = got.labels.cpu().numpy(), got.areas.cpu().numpy()
    np.testing.assert_array_equal(got_labels, labels, err_msg=str(what))
    np.testing.assert_array_equal(got_areas, areas, err_msg=str(what))
    assert got.counts.tolist() == counts.tolist(), what
    n, h, w = mask.shape
    assert got_areas.sum(axis=(1, 2)).tolist() == ((mask != 0) != holes).sum(axis=(1, 2)).tolist(), what
    np.testing.assert_array_equal(got_areas != 0, got_labels == 1 + np.arange(h * w, dtype=np.int64).reshape(1, h, w), err_msg=str(what))


# ------------------------------------------------------------------ 1. labels, areas, counts
@pytest.mark.parametrize("connectivity,holes", FORMS)
def test_components_are_the_restatement_on_the_main_shape(dev, connectivity, holes):
    for index, (names, mask) in enumerate(cn.batches(*MAIN)):
        got = mask_components(on(dev, mask), connectivity=connectivity, holes=holes)
        assert_components(got, cn.batch_components(*MAIN, index, connectivity, holes), mask, holes, (names, connectivity, holes))


@pytest.mark.parametrize("connectivity,holes", FORMS)
def test_components_are_the_restatement_on_small_and_degenerate_shapes(dev, connectivity, holes):
    for shape in SMALL:
        for index, (names, mask) in enumerate(cn.batches(*shape)):
            got = mask_components(on(dev, mask), connectivity=connectivity, holes=holes)
            assert_components(got, cn.batch_components(*shape, index, connectivity, holes), mask, holes, (shape, names, connectivity, holes))


def test_tiles_are_independent(dev):
    n, h, w = 4, 40, 70
    mask = np.stack([cn.random(h, w, 0.45, 70 + i) for i in range(n)])
    mask[:, -1] = 1      # tile i ends with a set row ...
    mask[:, 0] = 1       # ... and tile i + 1 begins with one: adjacent in memory, no neighbours
    mask[:, :, 0] = 1
    mask[:, :, -1] = 1
    for connectivity, holes in FORMS:
        batch = mask_components(on(dev, mask), connectivity=connectivity, holes=holes)
        assert_components(batch, cn.components(mask, connectivity, holes), mask, holes, (connectivity, holes))
        for i in range(n):
            single = mask_components(on(dev, mask[i:i + 1]), connectivity=connectivity, holes=holes)
            assert torch.equal(single.labels[0], batch.labels[i]) and torch.equal(single.areas[0], batch.areas[i]) and single.counts[0] == batch.counts[i]
        for call in (remove_small_objects, remove_small_holes):
            whole, whole_counts = call(on(dev, mask), 30, connectivity=connectivity)
            for i in range(n):
                part, part_counts = call(on(dev, mask[i:i + 1]), 30, connectivity=connectivity)
                assert torch.equal(part[0], whole[i]) and part_counts[0] == whole_counts[i]


# ------------------------------------------------------------------ 2. the filters
def check_filters(dev, mask: np.ndarray, connectivity: int, index_of, what) -> None:
    """min_area at 1, at A and A + 1 for the exact area A of one component per tile read from the restatement (objects and holes each
    their own), and at H * W + 1."""
    n, h, w = mask.shape
    x = on(dev, mask)
    inverse = on(dev, 1 - mask)
    for holes, call, restated in ((False, remove_small_objects, cn.objects_kept), (True, remove_small_holes, cn.holes_filled)):
        labels, areas, counts = index_of(connectivity, holes)
        present = sorted(set(areas[areas != 0].tolist()))
        chosen = present[len(present) // 2] if present else 1      # an area some component really has: the middle one of those present
        for min_area in (1, chosen, chosen + 1, h * w + 1):
            got, got_counts = call(x, min_area, connectivity=connectivity)
            assert got.dtype == torch.uint8 and got.shape == mask.shape and got_counts.dtype == torch.int64 and got_counts.shape == (n,), what
            got_np = got.cpu().numpy()
            np.testing.assert_array_equal(got_np, restated(labels, areas, min_area), err_msg=f"{what} holes={holes} min_area={min_area}")      # (the restatement's components, computed once)
            assert got_counts.tolist() == got_np.sum(axis=(1, 2), dtype=np.int64).tolist(), what
            # the complement identity, bit for bit
            other = (remove_small_objects if holes else remove_small_holes)(inverse, min_area, connectivity=connectivity)[0]
            assert torch.equal(got, 1 - other), (what, holes, min_area)
            kept = got_np if not holes else 1 - got_np      # 1 where a pixel of the labelled mask (the mask, or its complement) is still there
            if min_area == 1:
                np.testing.assert_array_equal(got_np, (mask != 0).astype(np.uint8))
            if min_area == h * w + 1:
                assert not kept.any(), (what, holes)
            if present:
                tile_index, first_pixel = np.argwhere(areas.reshape(n, -1) == chosen)[0]      # a component of exactly that area
                at = np.zeros(labels.shape, dtype=bool)
                at[tile_index] = labels[tile_index] == first_pixel + 1
                assert int(at.sum()) == chosen
                if min_area <= chosen:
                    assert kept[at].all(), (what, holes, min_area)      # an area equal to min_area stays
                else:
                    assert not kept[at].any(), (what, holes, min_area)


@pytest.mark.parametrize("connectivity", cn.CONNECTIVITIES)
def test_filters_are_the_restatement_on_the_main_shape(dev, connectivity):
    for index, (names, mask) in enumerate(cn.batches(*MAIN)):
        check_filters(dev, mask, connectivity, lambda c, holes, index=index: cn.batch_components(*MAIN, index, c, holes), names)


@pytest.mark.parametrize("connectivity", cn.CONNECTIVITIES)
def test_filters_are_the_restatement_on_small_and_degenerate_shapes(dev, connectivity):
    for shape in SMALL:
        for index, (names, mask) in enumerate(cn.batches(*shape)):
            check_filters(dev, mask, connectivity, lambda c, holes, shape=shape, index=index: cn.batch_components(*shape, index, c, holes), (shape, names))


def test_a_placed_component_is_kept_at_its_area_and_removed_one_above(dev):
    n, h, w = 2, 300, 150
    mask = np.zeros((n, h, w), dtype=np.uint8)
    mask[0, 250:262, 60:70] = 1      # 120 pixels across the corner of four blocks (rows 256, column 64)
    mask[0, 10:13, 10:13] = 1        # 9 pixels
    mask[0, 20, 20] = mask[0, 21, 21] = 1      # 2 pixels under 8, 1 + 1 under 4
    mask[1] = 1
    mask[1, 100:110, 30:42] = 0      # a hole of 120 pixels ...
    mask[1, 0:3, 0:3] = 0            # ... and glass of 9 pixels that touches the edge: a "hole" too
    x = on(dev, mask)
    for connectivity in cn.CONNECTIVITIES:
        for min_area, gone in ((120, [9, 2]), (121, [120, 9, 2]), (9, [2]), (10, [9, 2]), (2, [2] if connectivity == 4 else []), (3, [2])):
            got, counts = remove_small_objects(x, min_area, connectivity=connectivity)
            want = mask.copy()
            if 120 in gone:
                want[0, 250:262, 60:70] = 0
            if 9 in gone:
                want[0, 10:13, 10:13] = 0
            if 2 in gone:
                want[0, 20, 20] = want[0, 21, 21] = 0
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{connectivity} {min_area}")
            assert counts.tolist() == want.sum(axis=(1, 2), dtype=np.int64).tolist()
        for min_area, filled in ((9, []), (10, [9]), (120, [9]), (121, [9, 120])):
            got, counts = remove_small_holes(x, min_area, connectivity=connectivity)
            want = mask.copy()
            if 120 in filled:
                want[1, 100:110, 30:42] = 1
            if 9 in filled:
                want[1, 0:3, 0:3] = 1      # the hazard the docstring states: glass below the threshold is filled
            want[0] = cn.remove_small_holes(mask[:1], min_area, connectivity)[0]
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{connectivity} {min_area}")
            assert counts.tolist() == want.sum(axis=(1, 2), dtype=np.int64).tolist()


# ------------------------------------------------------------------ 3. input forms, degenerate masks
def test_input_forms(dev):
    n, h, w = 2, 70, 90
    mask = np.stack([cn.random(h, w, 0.5, 11), cn.frames(h, w)])
    base = mask_components(on(dev, mask))
    objects, holes = remove_small_objects(on(dev, mask), 12), remove_small_holes(on(dev, mask), 12)
    wide = np.zeros((n, h, 2 * w), dtype=np.uint8)
    wide[:, :, ::2] = mask
    wide[:, :, 1::2] = 1 - mask
    forms = {"bool": on(dev, mask).bool(), "n1hw": on(dev, mask).unsqueeze(1), "bool n1hw": on(dev, mask).bool().unsqueeze(1), "255": on(dev, mask * 255), "7": on(dev, mask * 7),
             "mixed": on(dev, mask * np.random.default_rng(1).integers(1, 256, mask.shape).astype(np.uint8)), "view": on(dev, wide)[:, :, ::2]}
    assert not forms["view"].is_contiguous()
    for name, x in forms.items():
        got = mask_components(x)
        assert got.labels.shape == (n, h, w), name
        assert torch.equal(got.labels, base.labels) and torch.equal(got.areas, base.areas) and torch.equal(got.counts, base.counts), name
        for call, want in ((remove_small_objects, objects), (remove_small_holes, holes)):
            out, counts = call(x, 12)
            assert out.shape == (n, h, w) and torch.equal(out, want[0]) and torch.equal(counts, want[1]), name
    assert_components(base, cn.components(mask), mask, False, "forms")


def test_all_set_all_clear_and_mixed_batches(dev):
    n, h, w = 3, 520, 200
    full, empty = np.ones((n, h, w), dtype=np.uint8), np.zeros((n, h, w), dtype=np.uint8)
    mixed = np.stack([full[0], empty[0], cn.random(h, w, 0.5, 21)])
    for connectivity in cn.CONNECTIVITIES:
        got = mask_components(on(dev, full), connectivity=connectivity)
        assert bool((got.labels == 1).all()) and got.counts.tolist() == [1] * n
        assert got.areas[:, 0, 0].tolist() == [h * w] * n and int(got.areas.sum()) == n * h * w
        got = mask_components(on(dev, empty), connectivity=connectivity)
        assert not bool(got.labels.any()) and not bool(got.areas.any()) and got.counts.tolist() == [0] * n
        got = mask_components(on(dev, empty), connectivity=connectivity, holes=True)
        assert bool((got.labels == 1).all()) and got.counts.tolist() == [1] * n and got.areas[:, 0, 0].tolist() == [h * w] * n
        for holes in (False, True):
            assert_components(mask_components(on(dev, mixed), connectivity=connectivity, holes=holes), cn.components(mixed, connectivity, holes), mixed, holes, "mixed")
        for min_area, stays in ((h * w, True), (h * w + 1, False)):
            out, counts = remove_small_objects(on(dev, full), min_area, connectivity=connectivity)
            assert bool((out == int(stays)).all()) and counts.tolist() == [h * w * stays] * n
            out, counts = remove_small_holes(on(dev, empty), min_area, connectivity=connectivity)      # glass smaller than the threshold is filled
            assert bool((out == int(not stays)).all()) and counts.tolist() == [h * w * (not stays)] * n
        out, counts = remove_small_objects(on(dev, mixed), 40, connectivity=connectivity)
        np.testing.assert_array_equal(out.cpu().numpy(), cn.remove_small_objects(mixed, 40, connectivity))
        assert counts[:2].tolist() == [h * w, 0]


# ------------------------------------------------------------------ 4. the Python pipeline
def test_refine_mask_and_otsu_mask(dev):
    n, h, w = 2, 90, 140
    mask = np.stack([cn.random(h, w, 0.55, 31), cn.random(h, w, 0.7, 32)])
    x = on(dev, mask * 255)
    # the defaults: today's bits through today's calls
    same, same_counts = refine_mask(x)
    assert torch.equal(same, on(dev, mask)) and same_counts.tolist() == mask.sum(axis=(1, 2), dtype=np.int64).tolist()
    today = mask_morphology(mask_morphology(x, "open", 1)[0], "close", 2)
    got = refine_mask(x, open_radius=1, close_radius=2)
    assert torch.equal(got[0], today[0]) and torch.equal(got[1], today[1])
    # the new arguments: small objects go, opening, closing, small holes go
    for connectivity in cn.CONNECTIVITIES:
        step = remove_small_objects(x, 25, connectivity=connectivity)
        step = mask_morphology(step[0], "open", 1, element="square")
        step = mask_morphology(step[0], "close", 2, element="square")
        step = remove_small_holes(step[0], 60, connectivity=connectivity)
        got = refine_mask(x, open_radius=1, close_radius=2, element="square", min_object_area=25, min_hole_area=60, connectivity=connectivity)
        assert torch.equal(got[0], step[0]) and torch.equal(got[1], step[1]), connectivity
        only_objects = refine_mask(x.unsqueeze(1), min_object_area=25, connectivity=connectivity)
        want = remove_small_objects(x, 25, connectivity=connectivity)
        assert torch.equal(only_objects[0], want[0]) and torch.equal(only_objects[1], want[1])
        np.testing.assert_array_equal(want[0].cpu().numpy(), cn.remove_small_objects(mask, 25, connectivity))
        only_holes = refine_mask(x, min_hole_area=60, connectivity=connectivity)
        want = remove_small_holes(x, 60, connectivity=connectivity)
        assert torch.equal(only_holes[0], want[0]) and torch.equal(only_holes[1], want[1])
    images = td.tiles_u8("stripes")[:3].contiguous().to(dev)
    plain = otsu_mask(images)
    by_hand = refine_mask(plain.mask, open_radius=2, close_radius=1)
    with_radii = otsu_mask(images, open_radius=2, close_radius=1)
    assert torch.equal(with_radii.mask, by_hand[0]) and torch.equal(with_radii.counts, by_hand[1]) and torch.equal(with_radii.thresholds, plain.thresholds)
    composed = remove_small_holes(mask_morphology(remove_small_objects(plain.mask, 20, connectivity=4)[0], "open", 1)[0], 50, connectivity=4)
    full = otsu_mask(images, open_radius=1, min_object_area=20, min_hole_area=50, connectivity=4)
    assert torch.equal(full.mask, composed[0]) and torch.equal(full.counts, composed[1]) and torch.equal(full.thresholds, plain.thresholds)


def test_real_tissue(dev):
    images = td.tiles_u8("real_256").to(dev)
    det = otsu_mask(images)
    mask = det.mask.cpu().numpy()
    assert 0 < int(mask.sum()) < mask.size
    for connectivity in cn.CONNECTIVITIES:
        objects, counts = remove_small_objects(det.mask, 64, connectivity=connectivity)
        want = cn.remove_small_objects(mask, 64, connectivity)
        np.testing.assert_array_equal(objects.cpu().numpy(), want)
        assert counts.tolist() == want.sum(axis=(1, 2), dtype=np.int64).tolist()
        holes, counts = remove_small_holes(det.mask, 64, connectivity=connectivity)
        want = cn.remove_small_holes(mask, 64, connectivity)
        np.testing.assert_array_equal(holes.cpu().numpy(), want)
        assert counts.tolist() == want.sum(axis=(1, 2), dtype=np.int64).tolist()
    assert_components(mask_components(det.mask), cn.components(mask), mask, False, "real_256")


# ------------------------------------------------------------------ 5. the raw C ABI, and a captured graph
def test_raw_abi_with_the_optional_outputs_null(dev):
    lib = _native.require()
    n, h, w = 2, 300, 100
    mask = np.stack([cn.random(h, w, 0.5, 41), cn.serpentine(h, w)])
    x = on(dev, mask)
    labels = torch.full((n, h, w), -7, dtype=torch.int32, device=dev)
    for connectivity in cn.CONNECTIVITIES:
        for invert in (0, 1):
            assert lib.sx_mask_components(x.data_ptr(), n, h, w, connectivity, invert, labels.data_ptr(), None, None, _native.stream_ptr(dev)) == 0
            np.testing.assert_array_equal(labels.cpu().numpy(), cn.components(mask, connectivity, bool(invert))[0])
    need = int(lib.sx_mask_components_workspace_bytes(n, h, w))
    workspace = torch.full((need + 3,), 0xA5, dtype=torch.uint8, device=dev)      # any contents, and not aligned
    out = torch.full((n, h, w), 9, dtype=torch.uint8, device=dev)
    for holes, restated in ((0, cn.remove_small_objects), (1, cn.remove_small_holes)):
        assert lib.sx_mask_area_filter(x.data_ptr(), out.data_ptr(), n, h, w, 4, holes, 1 << 40, workspace[3:].data_ptr(), None, _native.stream_ptr(dev)) == 0
        assert bool((out == holes).all())      # an int64 min_area above every area: all clear, or all set
        assert lib.sx_mask_area_filter(x.data_ptr(), out.data_ptr(), n, h, w, 4, holes, 7, workspace[3:].data_ptr(), None, _native.stream_ptr(dev)) == 0
        np.testing.assert_array_equal(out.cpu().numpy(), restated(mask, 7, 4))


def test_area_filter_in_a_captured_graph_reads_the_mask_at_replay(dev):
    lib = _native.require()
    n, h, w = 2, 300, 100
    first = np.stack([cn.random(h, w, 0.45, 51), cn.random(h, w, 0.6, 52)])
    new = np.stack([cn.random(h, w, 0.55, 53), cn.checkerboard(h, w)])
    x = on(dev, first)
    out, filled = torch.zeros((n, h, w), dtype=torch.uint8, device=dev), torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    counts, filled_counts = torch.zeros((n,), dtype=torch.int64, device=dev), torch.zeros((n,), dtype=torch.int64, device=dev)
    workspace = torch.empty((int(lib.sx_mask_components_workspace_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: one stream; the two calls share the workspace in stream order
        assert lib.sx_mask_area_filter(x.data_ptr(), out.data_ptr(), n, h, w, 8, 0, 30, workspace.data_ptr(), counts.data_ptr(), _native.stream_ptr(dev)) == 0
        assert lib.sx_mask_area_filter(out.data_ptr(), filled.data_ptr(), n, h, w, 4, 1, 20, workspace.data_ptr(), filled_counts.data_ptr(), _native.stream_ptr(dev)) == 0
    for mask in (first, new):
        x.copy_(on(dev, mask))
        graph.replay()
        torch.cuda.synchronize(dev)
        want = cn.remove_small_objects(mask, 30, 8)
        want_filled = cn.remove_small_holes(want, 20, 4)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        np.testing.assert_array_equal(filled.cpu().numpy(), want_filled)
        assert counts.tolist() == want.sum(axis=(1, 2), dtype=np.int64).tolist() and filled_counts.tolist() == want_filled.sum(axis=(1, 2), dtype=np.int64).tolist()
    assert not np.array_equal(cn.remove_small_objects(first, 30, 8), cn.remove_small_objects(new, 30, 8))
