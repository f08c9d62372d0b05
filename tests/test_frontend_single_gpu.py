"""The single-tile path the front ends share (stainx_amd/_frontend.py: ``image_batch``, ``call_mask``): a CHW tile with an (H, W) mask gives,
bit for bit, what the same tile gives as a (1, 3, H, W) batch with a (1, H, W) mask, squeezed -- through every front end that takes a tile.
One 40 x 56 tile: the width is no multiple of 16, so the kernels' scalar tail runs."""
from __future__ import annotations

import pytest
import torch

import stainx_amd as sx
from stainx_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = (torch.uint8, torch.float32)
LAB = (torch.tensor([150.0, 140.0, 120.0]), torch.tensor([20.0, 8.0, 9.0]))
HED = (torch.tensor([0.5, 0.3, 0.1]), torch.tensor([0.2, 0.1, 0.05]))
DISTRIBUTION = sx.StatisticsDistribution(LAB[0], LAB[1] / 4, LAB[1], LAB[1] / 4)
ROWS = torch.tensor([[0.03, 1.1, -0.02, 0.9, 0.05]])
F3, F2 = torch.tensor([[1.1, 0.9, 1.05]]), torch.tensor([[1.1, 0.9]])
B3, B2 = torch.tensor([[0.02, -0.03, 0.01]]), torch.tensor([[0.02, -0.03]])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tiles(dev):
    """dtype -> (the (1, 3, H, W) batch, its (1, H, W) masks): made once, never written.  "levels": the pixels darker than level 200 (on this
    tile: every pixel); "striped": those, less every third column, so that both sides of a mask are there."""
    u8 = synth.he_batch(1, 40, 56)
    out = {}
    for dtype in DTYPES:
        x = synth.as_dtype(u8, dtype).contiguous().to(dev)
        levels = (x.float().mean(dim=1) < (200.0 if dtype == torch.uint8 else 200.0 / 255)).to(torch.uint8).contiguous()
        striped = levels.clone()
        striped[:, :, ::3] = 0
        out[dtype] = (x, {"levels": levels, "striped": striped})
    return out


def on(dev, *tensors):
    return tuple(t.to(dev) for t in tensors)


# name -> (call(x, mask, dev, last), the result drops the batch axis, takes channel_axis=-1); a call builds its object anew: nothing is shared between the two forms
CALLS = {
    "ColorDeconvolution.apply": (lambda x, m, dev, last: sx.ColorDeconvolution("hed", channel_axis=-1 if last else 1).apply(x, *on(dev, F3, B3), mask=m), True, True),
    "ColorDeconvolution.quantify": (lambda x, m, dev, last: tuple(sx.ColorDeconvolution("hed", channel_axis=-1 if last else 1).quantify(x, mask=m))[:3], False, True),
    "ColorDeconvolution.estimate": (lambda x, m, dev, last: tuple(sx.ColorDeconvolution("hed", channel_axis=-1 if last else 1).estimate(x, mask=m)), False, True),
    "ColorDeconvolution.match": (lambda x, m, dev, last: sx.ColorDeconvolution("hed", channel_axis=-1 if last else 1).match(x, on(dev, *HED), on(dev, HED[0] * 1.2, HED[1] * 0.8), mask=m), True, True),
    "HEDAugment": (lambda x, m, dev, last: sx.HEDAugment()(x, *on(dev, F3, B3), mask=m), True, False),
    "adjust_hsv": (lambda x, m, dev, last: sx.adjust_hsv(x, ROWS.to(dev), mask=m, channel_axis=-1 if last else 1), True, True),
    "HSVAugment": (lambda x, m, dev, last: sx.HSVAugment()(x, ROWS.to(dev), mask=m), True, False),
    "MacenkoAugment": (lambda x, m, dev, last: sx.MacenkoAugment()(x, *on(dev, F2, B2), mask=m), True, False),
    "StatisticsAugment lab": (lambda x, m, dev, last: sx.StatisticsAugment(DISTRIBUTION, "lab")(x, on(dev, *LAB), mask=m), True, False),
    "StatisticsAugment hed": (lambda x, m, dev, last: sx.StatisticsAugment(DISTRIBUTION, "hed")(x, on(dev, *HED), mask=m), True, False),
    "LuminosityStandardizer": (lambda x, m, dev, last: sx.LuminosityStandardizer()(x, mask=m), True, False),
}


def same(single, batched, squeezed):
    if isinstance(single, tuple):
        assert len(single) == len(batched)
        return all(same(s, b, squeezed) for s, b in zip(single, batched))
    assert tuple(single.shape) == tuple(batched.shape[1:] if squeezed else batched.shape), (tuple(single.shape), tuple(batched.shape))
    return torch.equal(single, batched.squeeze(0) if squeezed else batched)


@pytest.mark.parametrize("which", ("levels", "striped"))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("name", CALLS)
def test_a_masked_tile_is_its_batch_of_one(dev, tiles, name, dtype, which):
    call, squeezed, _ = CALLS[name]
    x, mask = tiles[dtype][0], tiles[dtype][1][which]
    assert int(mask.sum()) > 0
    assert same(call(x[0], mask[0], dev, False), call(x, mask, dev, False), squeezed)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("name", [name for name, (_, _, nhwc) in CALLS.items() if nhwc])
def test_an_unmasked_channels_last_tile_is_its_batch_of_one(dev, tiles, name, dtype):
    call, squeezed, _ = CALLS[name]
    x = tiles[dtype][0].permute(0, 2, 3, 1).contiguous()
    assert same(call(x[0], None, dev, True), call(x, None, dev, True), squeezed)
