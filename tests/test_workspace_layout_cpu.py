"""The Macenko workspace sizes as the C ABI reports them (pure host functions, no GPU): one walk over the areas (macenko.hip:
workspace_layout) yields both the pointers and the end of every level, and these are the relations its answers must keep -- the part of
the buffer one call needs is a prefix of the whole, every level ends on a 256-byte boundary, and a call sent to the four passes needs
what SX_MACENKO_CLASSIC needs.  The Reinhard sizes come from one walk of their own (reinhard.hip: workspace_layout): pooled, per tile
and masked calls keep the pooled areas in front, and the relations between their sizes are those below."""
from __future__ import annotations

import itertools

import pytest

from stainx_amd import _native

CLASSIC, CHANNELS_LAST, SAMPLED = 16, 2, 4
DTYPES = range(5)
BATCHES = (1, 2, 16, 64, 256)
TILES = ((16, 16), (47, 49), (48, 48), (128, 128), (224, 224), (512, 512), (724, 724), (1024, 1024), (2048, 2048))
FLAG_SETS = (0, CLASSIC, CHANNELS_LAST, SAMPLED)


@pytest.fixture(scope="module")
def lib():
    return _native.require()


@pytest.mark.parametrize("n", BATCHES)
def test_one_call_needs_a_prefix_of_the_whole(lib, n):
    for (h, w), dtype, flags in itertools.product(TILES, DTYPES, FLAG_SETS):
        whole, part = lib.sx_macenko_workspace_bytes(n, h, w), lib.sx_macenko_workspace_bytes_for(dtype, n, h, w, flags)
        assert 0 < part <= whole, (dtype, n, h, w, flags, part, whole)
        assert part % 256 == 0 and whole % 256 == 0, (dtype, n, h, w, flags, part, whole)


@pytest.mark.parametrize("n", BATCHES)
def test_four_pass_calls_need_the_classic_size(lib, n):
    for (h, w), dtype, flags in itertools.product(TILES, DTYPES, FLAG_SETS):
        classic = lib.sx_macenko_workspace_bytes_for(dtype, n, h, w, flags | CLASSIC)
        part, form = lib.sx_macenko_workspace_bytes_for(dtype, n, h, w, flags), lib.sx_macenko_form(dtype, n, h, w, flags)
        assert lib.sx_macenko_form(dtype, n, h, w, flags | CLASSIC) == 0
        assert part >= classic, (dtype, n, h, w, flags, part, classic)      # (the classic size is the base level: a prefix of every form's)
        if part == classic:
            assert form == 0, (dtype, n, h, w, flags, form)
        if form == 0:
            assert part == classic, (dtype, n, h, w, flags, part, classic)


@pytest.mark.parametrize("n,h,w", [(0, 16, 16), (-1, 16, 16), (4, 0, 16), (4, 16, -3), (0, 0, 0)])
def test_non_positive_sizes_give_zero(lib, n, h, w):
    assert lib.sx_macenko_workspace_bytes(n, h, w) == 0
    for dtype, flags in itertools.product(DTYPES, FLAG_SETS):
        assert lib.sx_macenko_workspace_bytes_for(dtype, n, h, w, flags) == 0
        assert lib.sx_macenko_form(dtype, n, h, w, flags) == 0


@pytest.mark.parametrize("n", BATCHES + (4096, 5000))
def test_reinhard_and_histogram_matching_sizes(lib, n):
    f32 = 3
    for (h, w), dtype in itertools.product(TILES, DTYPES):
        plain, sized, tiles = lib.sx_reinhard_workspace_bytes(n, h, w), lib.sx_reinhard_workspace_bytes_for(dtype, n, h, w), lib.sx_reinhard_tiles_workspace_bytes(dtype, n, h, w)
        masked = lib.sx_reinhard_masked_workspace_bytes(dtype, n, h, w)
        for size in (plain, sized, tiles, masked):
            assert size > 0 and size % 256 == 0, (dtype, n, h, w, size)
        assert plain <= sized <= tiles, (dtype, n, h, w, plain, sized, tiles)
        coded = dtype == f32 and (h * w) % 4 == 0 and n * h * w >= 1 << 20      # (the codes of a float32 batch lie behind the other areas)
        assert (sized > plain) == coded, (dtype, n, h, w, plain, sized)
        assert (tiles > lib.sx_reinhard_tiles_workspace_bytes(0, n, h, w)) == coded, (dtype, n, h, w, tiles)
        assert masked >= lib.sx_reinhard_tiles_workspace_bytes(0, n, h, w), (dtype, n, h, w, masked)      # (NOT the float32 per-tile size: the masked calls keep no codes)
    for h, w in TILES:
        pooled, tiles, masked = lib.sx_hm_workspace_bytes(n, h, w), lib.sx_hm_tiles_workspace_bytes(n, h, w), lib.sx_hm_masked_workspace_bytes(n, h, w)
        assert 0 < pooled < tiles < masked, (n, h, w, pooled, tiles, masked)
