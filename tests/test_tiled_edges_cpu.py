"""What tests/_tiled_edges.py claims, checked without a GPU: the block sizes it restates are the sources' own constants; every shape is
classified as the table says (pack path, blocks across and down, columns and rows of the last block; JPEG: W mod 8 and the regions); the
blur's sigma set reaches every radius 0..16 and both sides of every border of the radius rule; a float32 model of the taps, built by the
header's rule, stays within a quarter of the impulse bound of the float64 taps; the quality set reaches table entries 1 and 255 and both
sides of the branch at 50; the quality rule's rows are what ``min((int)q, 100)`` says; and the numpy restatement of the JPEG round trip
equals a live Pillow on the new shapes (skipped where Pillow is missing, as tests/test_jpeg_cpu.py's comparison is)."""
from __future__ import annotations

import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _blur_numpy as bn
from tests import _focus_numpy as fn
from tests import _jpeg_numpy as jn
from tests import _tiled_edges as te

CSRC = Path(__file__).resolve().parents[1] / "stainx_amd" / "csrc"


# ------------------------------------------------------------------ 1. the shape rule
def test_block_sizes_are_the_sources_constants():
    for name, constants in te.CONSTANTS.items():
        text = (CSRC / name).read_text()
        for constant, value in constants.items():
            found = re.search(r"constexpr int " + constant + r" = (\d+);", text)
            assert found and int(found.group(1)) == value, (name, constant)
    assert "kWarpSide" in (CSRC / "elastic.hpp").read_text()      # (the elastic warp cuts the same blocks)
    assert te.BLOCKS["blur"] == (te.CONSTANTS["blur.hpp"]["kBlurSide"],) * 2 and te.BLOCKS["warp"] == (te.CONSTANTS["warp.hpp"]["kWarpSide"],) * 2
    assert te.BLOCKS["focus"] == (te.CONSTANTS["focus.hpp"]["kFocusRows"], te.CONSTANTS["focus.hpp"]["kFocusCols"]) == fn.BLOCK
    jpeg = te.CONSTANTS["jpeg_block.hpp"]
    assert te.BLOCKS["jpeg444"] == (jpeg["kJpegRegionH444"], jpeg["kJpegRegionW"]) and te.BLOCKS["jpeg420"] == (jpeg["kJpegRegionH420"], jpeg["kJpegRegionW"])
    assert bn.MAX_RADIUS == te.CONSTANTS["blur.hpp"]["kBlurMaxRadius"]


@pytest.mark.parametrize("kernel", ["blur", "focus", "warp"])
def test_every_shape_is_ragged_on_the_pack_path(kernel):
    block = te.BLOCKS[kernel]
    for shape, (across, down, last_cols, last_rows) in te.SHAPES[kernel].items():
        h, w = shape[-2:]
        c = te.classify(h, w, block)
        assert c["pack"] and c["ragged"] and w % 4 == 0 and w % block[1] != 0, (kernel, shape)
        assert (c["across"], c["down"], c["last_cols"], c["last_rows"]) == (across, down, last_cols, last_rows), (kernel, shape, c)
        assert c["last_cols"] < block[1] and c["last_cols"] % 4 == 0      # packs up to the tile's edge, none across it
        assert h * w < te.MAX_PIXELS, shape


def test_the_blur_shapes_reach_each_case():
    shapes = te.BLUR_SHAPES
    assert any(v[0] == 1 and v[2] < bn.MAX_RADIUS for v in shapes.values())                 # a single ragged block narrower than R
    assert any(v[0] == 2 and v[2] == 4 for v in shapes.values()) and any(v[0] == 3 and v[2] == 4 for v in shapes.values())      # 4 columns behind one and behind two full blocks
    assert any(v[1] > 1 and v[3] < 64 and v[0] > 1 for v in shapes.values())                # a ragged block row as well
    assert all(te.classify(*s, te.BLOCKS["blur"])["ragged"] for s in te.IMPULSE_SHAPES)
    # ... which the shape list of the kernels' own test files never does: there every pack width is a whole number of blocks
    inherited = ((1, 1), (1, 7), (2, 2), (5, 3), (33, 31), (64, 64), (65, 130), (144, 128))
    for block in ("blur", "warp"):
        assert not any(te.classify(h, w, te.BLOCKS[block])["ragged"] for h, w in inherited), block


def test_the_jpeg_shapes_reach_each_case():
    for (h, w), (mod8, across, down444, down420, last_cols) in te.JPEG_SHAPES.items():
        c444, c420 = te.classify(h, w, te.BLOCKS["jpeg444"]), te.classify(h, w, te.BLOCKS["jpeg420"])
        assert c444["pack"] and c444["ragged"] and h * w < te.MAX_PIXELS, (h, w)
        assert (w % 8, c444["across"], c444["down"], c420["down"], c444["last_cols"]) == (mod8, across, down444, down420, last_cols), (h, w)
        assert c420["across"] == across
    values = list(te.JPEG_SHAPES.values())
    assert sum(v[0] == 4 for v in values) >= 6                               # W = 4 mod 8: the 8-column block extension meets the pack test
    assert any(v[1] == 2 for v in values) and any(v[1] == 3 for v in values)      # two and three regions across (three: a chroma halo of real samples on both sides)
    assert any(v[2] >= 2 for v in values) and any(v[3] == 2 for v in values)      # two regions down in each subsampling
    assert any(v[0] == 4 and v[1] == 2 for v in values)                      # a second region whose only pack is half a block
    c = te.classify(*te.QUALITY_SHAPE, te.BLOCKS["jpeg420"])
    assert c["pack"] and te.QUALITY_SHAPE[1] % 16 == 8                       # one and a half MCUs wide


# ------------------------------------------------------------------ 2. blur: radii, borders, taps
def test_the_sigma_set_reaches_every_radius_and_both_sides_of_every_border():
    sigmas = te.radius_sigmas()
    assert len(sigmas) == 66
    assert {bn.radius(s) for s in sigmas} == set(range(17))
    for k, s in enumerate(te.border_sigmas()):
        assert float(np.float32(s)) == s and 4.0 * s + 0.5 == k + 1                      # exact in float32, and exactly on the border
        assert bn.radius(s) == k + 1 and bn.radius(te.below(s)) == k and bn.radius(te.above(s)) == k + 1, k
        assert float(te.below(s)) in sigmas and s in sigmas and float(te.above(s)) in sigmas
    assert all(bn.radius(r / 4.0) == r for r in range(1, 17))
    assert bn.radius(te.above(4.0)) == 16 and float(te.above(4.0)) in sigmas
    assert {bn.radius(s) for s in te.impulse_sigmas()} == set(range(17))
    assert tuple(bn.radius(s) for s in te.RAGGED_SIGMAS) == te.RAGGED_RADII
    x, tile_sigmas, places = te.impulse_tiles((9, 36))
    assert x.shape[0] == len(tile_sigmas) == len(places) == 2 * len(te.impulse_sigmas()) and float(x.sum()) == 3 * x.shape[0] and x.dtype == torch.float32
    # the impulse places of the large shape: a block's middle at least 16 from every border and seam, a block corner, the ragged block, tile corners
    (middle, corner, ragged), (first, last, _) = te.impulse_places((100, 132))
    assert all(16 <= v % 64 < 48 for v in middle) and corner == (63, 64) and ragged[1] == 132 - 3 and ragged[1] // 64 == 2 and first == (0, 0) and last == (99, 131)


def test_float32_taps_by_the_headers_rule_stay_within_a_quarter_of_the_impulse_bound():
    assert te.REL == 2.0**-15 and te.REL <= 1e-4
    worst = 0.0
    for s in sorted(set(te.radius_sigmas() + te.impulse_sigmas())):
        r = bn.radius(s)
        if r == 0:
            continue
        w64, w32 = bn.taps(s)[r:], te.taps32(s)
        assert w32.dtype == np.float32 and w32.shape == w64.shape == (r + 1,) and (w32 > 0).all()
        worst = max(worst, float(np.abs(w32.astype(np.float64) / w64 - 1.0).max()))
        # a product of two taps, as the impulse response holds them
        worst = max(worst, float(np.abs(np.outer(w32, w32).astype(np.float64) / np.outer(w64, w64) - 1.0).max()))
    print(f"float32 taps (and products of two) against float64 over the sigma set: worst relative error {worst:.3e} (a quarter of REL: {te.REL / 4:.3e})")
    assert worst <= te.REL / 4


def test_blur_references_are_shared_and_read_only():
    a = te.blur_reference(torch.uint8, (3, 12), te.RAGGED_SIGMAS)
    assert a is te.blur_reference(torch.uint8, (3, 12), te.RAGGED_SIGMAS) and not a.flags.writeable and a.shape == (5, 3, 3, 12)
    x = te.blur_tiles(torch.uint8, (3, 12), 5)
    assert np.array_equal(a[3], x[3].numpy().astype(np.float64))      # the NaN sigma: a copy
    assert np.array_equal(a[2], bn.blur64(x[2].numpy().astype(np.float64), 4.0)) and np.array_equal(a[4], bn.blur64(x[4].numpy().astype(np.float64), 4.0))      # 7.0 is 4.0


# ------------------------------------------------------------------ 3. JPEG: tables, the rule, Pillow
def test_the_quality_set_reaches_the_tables_corners():
    qualities = te.every_quality()
    assert qualities == tuple(float(q) for q in range(1, 101))
    tables = [np.stack(jn.tables(q)) for q in qualities]
    assert len({t.tobytes() for t in tables}) == 100                                         # a hundred different tables
    assert any((t == 1).any() for t in tables) and any((t == 255).any() for t in tables)     # both clamps
    assert (tables[0] == 255).all() and (tables[99] == 1).all()
    assert any((t == 255).any() and (t < 255).any() for t in tables)                         # the upper clamp biting on a part of a table only
    assert any(q < 50 for q in qualities) and any(q >= 50 for q in qualities) and 49.0 in qualities and 50.0 in qualities      # both sides of the branch
    tiles = te.jpeg_tiles(te.QUALITY_SHAPE, 100)
    assert tiles.shape == (100, 3, 16, 24) and not tiles.flags.writeable
    noise, real = tiles[0::2].astype(np.int64), tiles[1::2].astype(np.int64)
    assert np.abs(np.diff(real, axis=-1)).mean() < 0.25 * np.abs(np.diff(noise, axis=-1)).mean()      # the real crops are smooth: small coefficients
    assert len({t.tobytes() for t in tiles}) == 100


def test_the_quality_rules_rows():
    assert len(te.RULE_ROWS) == len(te.RULE_QUALITY) == 19
    for q, want in zip(te.RULE_ROWS, te.RULE_QUALITY):
        q32 = np.float32(q)
        expect = min(int(q32), 100) if np.isfinite(q32) and q32 >= 1 else 0
        assert expect == want, (q, expect, want)
    assert np.isfinite(np.float32(te.FLT_MAX)) and np.float32(3.2e38) > np.float32(3.0e38) and np.isfinite(np.float32(3.2e38))
    # the restatement follows the rule on these rows: a finite quality however large is 100, the rest keep their levels
    tiles = te.jpeg_tiles(te.RULE_SHAPE, len(te.RULE_ROWS))
    for sub in (0, 2):
        got = jn.roundtrip(tiles, te.RULE_ROWS, sub)
        for t, quality in enumerate(te.RULE_QUALITY):
            want = tiles[t] if quality == 0 else jn.roundtrip_levels(tiles[t], quality, sub)
            assert np.array_equal(got[t], want), (t, quality, sub)
            assert (quality == 0) == np.array_equal(got[t], tiles[t])


def test_restatement_equals_a_live_pillow_on_the_new_shapes():
    image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2027)
    for h, w in tuple(te.JPEG_SHAPES) + (te.QUALITY_SHAPE, te.RULE_SHAPE):
        tile = rng.integers(0, 256, size=(3, h, w), dtype=np.uint8)
        for q in (10, 50, 95):
            for s in (0, 2):
                buffer = io.BytesIO()
                image.fromarray(np.ascontiguousarray(tile.transpose(1, 2, 0)), "RGB").save(buffer, "JPEG", quality=q, subsampling=s)
                buffer.seek(0)
                want = np.asarray(image.open(buffer).convert("RGB")).transpose(2, 0, 1)
                assert np.array_equal(jn.roundtrip_levels(tile, q, s), want), (h, w, q, s)
    tiles = te.jpeg_tiles(te.QUALITY_SHAPE, 100)      # every quality, on the tiles the GPU test uses
    for t, q in enumerate(te.every_quality()):
        for s in (0, 2):
            buffer = io.BytesIO()
            image.fromarray(np.ascontiguousarray(tiles[t].transpose(1, 2, 0)), "RGB").save(buffer, "JPEG", quality=int(q), subsampling=s)
            buffer.seek(0)
            assert np.array_equal(jn.roundtrip_levels(tiles[t], q, s), np.asarray(image.open(buffer).convert("RGB")).transpose(2, 0, 1)), (q, s)


# ------------------------------------------------------------------ 5. the warps' rows and special values
def test_the_copy_path_rows_and_special_values():
    from tests import _warp_numpy as wn

    rows = np.asarray(te.LEFT_ROWS, dtype=np.float32)
    assert np.isnan(rows[0]).all() and np.isinf(rows[1]).any() and not np.isnan(rows[1]).any() and np.isfinite(rows[2]).all()
    for h, w in te.WARP_SHAPES:
        anchor = wn.anchor_row(h, w, h, w)
        for r in (0, 1):      # a row that is not finite becomes the anchor row: equal sizes, the identity -- a copy
            assert np.array_equal(wn.effective_row(te.LEFT_ROWS[r], h, w, h, w), anchor) and np.array_equal(anchor, np.asarray(wn.IDENTITY, dtype=anchor.dtype))
        assert np.array_equal(wn.effective_row(te.LEFT_ROWS[2], h, w, h, w), rows[2])
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        x = te.with_specials(torch.full((3, 3, 5, 36), 0.5, dtype=dtype))
        assert bool(torch.isinf(x).any()) and bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any())      # infinities and -0.0
        assert bool(torch.isnan(x).any()) == (dtype != torch.float64)
