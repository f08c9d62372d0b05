"""The estimate stage's single key sweep (macenko_twopass.hpp) held to the four passes bit for bit, on the PRODUCT library.

The stage bins the keys of a slot while it makes them: the range of the 256 level-0 bins is known before the keys (an angle
slot: the keys of the two mapped bracket boundaries, on an open side the prior's stand-in direction; a concentration slot:
[k_floor, k_ceil]), keys beyond it share the end bins, and select_slot_keys goes on from the filled histogram.  What can go
wrong is a candidate visited twice or not at all for some candidate count, a level-0 histogram that disagrees with the bins
the selection goes on from, and an answer inside an end bin or a crowded bin.  Every case asserts what
test_product_forms_gpu.py's _forms_agree asserts: the default call and SX_MACENKO_CLASSIC give the same output bytes and the
same per-tile intermediates (phi keys, max_c, he, ...).

Mutation checks (built by hand, MI355X): a candidate walk that skips one record (record 5 of every slot never visited) and a
level-0 range one bin too narrow in the filling sweep only (scale * 256 / 255 there) each fail all 12 cases of this module.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import synth
from tests.test_product_forms_gpu import F32, U8, _forms_agree, _report, _tissue, dev, lib, ref  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

K_LDS_KEYS = 16384      # macenko.hip kLdsKeys: keys of a slot the stage keeps in LDS; candidates beyond it spill to memory


def _prior_sample_mask(h: int, w: int) -> np.ndarray:
    """True where prior_kernel samples the tile (prior_fetch: unit u takes one 16-pixel sector of cell u at a hashed offset)."""
    pixels = h * w
    n_sectors = pixels // 16
    units = min(max(n_sectors // 4, min(n_sectors, 64)), 1024)
    step = (n_sectors << 16) // units
    mask = np.zeros(pixels, dtype=bool)
    for u in range(units):
        start = (u * step) >> 16
        width = (((u + 1) * step) >> 16) - start
        sector = start + (((((u * 0x9E3779B1) & 0xFFFFFFFF) >> 16) * width) >> 16)
        mask[16 * sector:16 * sector + 16] = True
    return mask.reshape(h, w)


def _stain_colours(n: int, stain: int, seed: int) -> torch.Tensor:
    """n uint8 colours of (almost) one pure stain: beyond every mixed pixel of a synthetic tile in angle, all different in amount."""
    rng = np.random.default_rng(seed)
    he = np.asarray(synth.HE_REF, dtype=np.float64)
    main = rng.uniform(0.9, 1.5, n) if stain == 0 else rng.uniform(0.7, 1.1, n)
    other = rng.uniform(0.0, 0.02, n)
    conc = np.stack([main, other] if stain == 0 else [other, main])
    od = he @ conc
    return torch.from_numpy(np.clip(np.round(240.0 * np.exp(-od)), 0, 255).astype(np.uint8))      # (3, n)


def _plant_unsampled(tile: torch.Tensor, n: int, stain: int, seed: int) -> None:
    """n pixels of one pure stain at places the prior does NOT look at: the tile's wanted angle percentile then lies beyond the
    extreme of the prior's sample -- outside the range the stage binned its keys over, in an end bin."""
    h, w = tile.shape[1:]
    free = np.flatnonzero(~_prior_sample_mask(h, w).reshape(-1))
    at = torch.from_numpy(np.random.default_rng(seed).choice(free, n, replace=False))
    tile.view(3, -1)[:, at] = _stain_colours(n, stain, seed + 1)


STRESS = {2: "one colour", 4: "two colours", 6: "a few hundred colours", 8: "1 % slot beyond the sample (end bin)",
          10: "99 % slot beyond the sample (end bin)", 12: "tied block larger than the LDS key array", 13: "the same at the other end"}


def _stress_batch() -> torch.Tensor:
    x = _tissue(16, 512, 512)
    x[2] = torch.tensor([150, 90, 160], dtype=torch.uint8).view(3, 1, 1)
    x[4] = torch.where((torch.arange(512).view(1, 512, 1) // 7 + torch.arange(512).view(1, 1, 512) // 5) % 3 == 0,
                       torch.tensor([120, 60, 140], dtype=torch.uint8).view(3, 1, 1), torch.tensor([190, 120, 170], dtype=torch.uint8).view(3, 1, 1))
    x[6] = (x[6] // 6) * 6 + 2
    assert 100 < torch.unique(x[6].view(3, -1).T, dim=0).shape[0] < 600
    _plant_unsampled(x[8], 3500, 0, 81)        # 1.3 % of the tile: more than the 1 % the percentile cuts off
    _plant_unsampled(x[10], 3500, 1, 82)
    # 22 000 pixels (8.4 %) of ONE pure-stain colour, sampled or not: the percentile is that colour, and every one of them is a candidate
    for t, stain in ((12, 0), (13, 1)):
        x[t].view(3, -1)[:, 5000:27000] = _stain_colours(1, stain, 90 + t)
    return x


@pytest.fixture(scope="module")
def real_images(golden):
    return torch.from_numpy(golden("g11_real_images.npz")["images_u8"])


def test_config2_batch_keeps_every_slot_on_the_single_sweep(lib, dev, ref):
    """bench.py's first batch.  Not a measurement: the running slow-slot count must not move, as on the four-launch form before."""
    x = synth.as_dtype(synth.he_batch(64, 512, 512, seed0=1000), F32)
    r = _forms_agree(lib, ref, x.to(dev), what="config 2")
    _report("config 2", r)
    assert r.slow == 0 and int((r.params["fell_back"] & 15).sum()) == 0
    assert int(r.params["n_candidates"].min()) > 0


@pytest.mark.parametrize("dt", [F32, U8], ids=["f32", "u8"])
def test_real_quadrants_all_six_images(lib, dev, ref, real_images, dt):
    quads = torch.stack([real_images[i, :, y:y + 512, x:x + 512] for i in range(6) for y in (0, 512) for x in (0, 512)]).contiguous()
    assert quads.shape[0] == 24
    r = _forms_agree(lib, ref, synth.as_dtype(quads, dt).to(dev), what=("24 quadrants", dt))
    _report(f"24 real quadrants {dt}", r)


@pytest.mark.parametrize("dt", [F32, U8], ids=["f32", "u8"])
def test_tiles_that_stress_a_prebinned_histogram(lib, dev, ref, dt):
    r = _forms_agree(lib, ref, synth.as_dtype(_stress_batch(), dt).to(dev), what=("stress", dt))
    _report(f"stress {dt}", r)
    for t, name in STRESS.items():
        print(f"  tile {t:2d} ({name}): fell_back {int(r.params['fell_back'][t]) & 15:#x}, candidates {r.params['n_candidates'][t].tolist()}")
    # the tissue tiles between the built ones stay on the speculative path
    plain = [t for t in range(16) if t not in STRESS]
    assert int((r.params["fell_back"][plain] & 15).sum()) == 0


def test_more_candidates_than_the_lds_key_array(lib, dev, ref):
    """A slot whose candidates exceed kLdsKeys, selected on the speculative path: the keys beyond the array are written to and read
    back from memory."""
    r = _forms_agree(lib, ref, synth.as_dtype(_stress_batch(), F32).to(dev), what="spill")
    spilled = [(t, s) for t in (12, 13) for s in range(4)
               if int(r.params["n_candidates"][t, s]) > K_LDS_KEYS and not (int(r.params["fell_back"][t]) >> s) & 1]
    print("slots with spilled keys on the speculative path:", spilled, r.params["n_candidates"][[12, 13]].tolist())
    assert spilled


SIZES = [(40, 360, 360, F32), (24, 384, 512, F32), (16, 512, 512, F32), (36, 372, 380, F32), (16, 512, 512, U8), (32, 364, 364, U8)]


@pytest.mark.parametrize("n,h,w,dt", SIZES, ids=lambda v: str(v).split(".")[-1])
def test_tile_sizes_with_other_candidate_counts(lib, dev, ref, n, h, w, dt):
    """Every tile has its own candidate counts (hundreds of different n over the cases): the walk must visit each of the n
    records exactly once whatever n is modulo the workgroup's 1024 threads."""
    r = _forms_agree(lib, ref, synth.as_dtype(_tissue(n, h, w), dt).to(dev), what=(n, h, w, dt))
    _report(f"{(n, h, w)} {dt}", r)
    c = r.params["n_candidates"]
    print(f"  candidate counts mod 1024: {torch.unique(c % 1024).numel()} different residues, range {int(c.min())} .. {int(c.max())}")
