"""``Vahadane`` on the GPU, through its public surface: transform / fit_transform / separate against the steps they are made of (bit for
bit), a non-default stream, a captured graph replayed once, and ``MacenkoAugment`` with a Vahadane estimate as its source."""
from __future__ import annotations

import pytest
import torch

from stainx_amd import Macenko, MacenkoAugment, StainEstimate, Vahadane, synth
from tests import _vahadane_numpy as vn
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def real_u8():
    images = vn.real_images()
    return torch.from_numpy(images[:4, :, 300:428, 400:528].copy()), torch.from_numpy(images[5:6, :, 200:392, 100:292].copy())      # tiles (4, 128 x 128), a reference (1, 192 x 192)


def equal_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
@pytest.mark.parametrize("mode", ["luminosity", None])
def test_transform_fit_transform_and_separate_are_their_steps(dev, real_u8, name, mode):
    tiles, reference = (synth.as_dtype(t, TORCH_DTYPES[name]).to(dev) for t in real_u8)
    norm = Vahadane(device=dev, iterations=8, mask=mode).fit(reference)
    assert tuple(norm._stain_matrix.shape) == (3, 2) and tuple(norm._target_max_conc.shape) == (2,)
    pooled = norm.estimate(reference, pooled=True)
    assert equal_bits(norm._stain_matrix, pooled.stain_matrices[0]) and equal_bits(norm._target_max_conc, pooled.max_concentrations[0]) and pooled.tissue_pixels is None
    est = norm.estimate(tiles)
    assert isinstance(est, StainEstimate) and tuple(est.stain_matrices.shape) == (4, 3, 2) and tuple(est.max_concentrations.shape) == (4, 2)
    out = norm.transform(tiles)
    assert out.dtype == tiles.dtype and equal_bits(out, norm.apply(tiles, est))
    both = Vahadane(device=dev, iterations=8, mask=mode)
    assert equal_bits(both.fit_transform(tiles), Vahadane(device=dev, iterations=8, mask=mode).fit(tiles).transform(tiles))
    for fitted in (norm, Vahadane(device=dev, iterations=8, mask=mode)):      # to the reference, and in the tiles' own bases
        mine = fitted.separate(tiles, concentrations=True)
        steps = fitted.separate(tiles, concentrations=True, source=est)
        for a, b in zip(mine, steps):
            assert (a is None and b is None) or equal_bits(a, b)
    # a Macenko estimate as the initial dictionary, one per tile
    seeded = Vahadane(device=dev, iterations=8, mask=mode, init=Macenko(device=dev).estimate(tiles)).estimate(tiles)
    columns = seeded.stain_matrices.double()      # (another start, eight rounds: another point on the way; what holds is the constraint set)
    assert torch.isfinite(columns).all() and bool((columns >= 0).all()) and torch.allclose((columns ** 2).sum(dim=1), torch.ones(4, 2, dtype=torch.float64, device=dev), atol=1e-6)
    assert bool((columns[:, 0, 0] >= columns[:, 0, 1]).all())      # haematoxylin first


def test_side_stream_and_captured_graph(dev, real_u8):
    tiles, reference = (t.to(dev) for t in real_u8)
    norm = Vahadane(device=dev, iterations=5).fit(reference)
    want_est, want_out = norm.estimate(tiles), norm.transform(tiles)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        est, out = norm.estimate(tiles), norm.transform(tiles)      # (also warms the side stream's workspace up for the capture)
    side.synchronize()
    assert equal_bits(est.stain_matrices, want_est.stain_matrices) and equal_bits(est.max_concentrations, want_est.max_concentrations) and equal_bits(out, want_out)
    static = tiles.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):      # one stream: no parallel branches
            g_est = norm.estimate(static)
            g_out = norm.transform(static)
    static.copy_(torch.flip(tiles, dims=(0,)))      # the replay reads what the buffer holds now
    graph.replay()
    torch.cuda.synchronize(dev)
    assert equal_bits(g_est.stain_matrices, torch.flip(want_est.stain_matrices, dims=(0,))) and equal_bits(g_est.max_concentrations, torch.flip(want_est.max_concentrations, dims=(0,)))
    assert equal_bits(g_out, torch.flip(want_out, dims=(0,)))


def test_macenko_augment_takes_a_vahadane_estimate(dev, real_u8):
    tiles, reference = (t.to(dev) for t in real_u8)
    norm = Vahadane(device=dev, iterations=5).fit(reference)
    est = norm.estimate(tiles)
    module = MacenkoAugment(0.0, 0.0, source=est, normalizer=norm, normalize_to_0_1=False)
    out = module(tiles)
    assert out.shape == tiles.shape and out.dtype == torch.uint8
    plain = Vahadane(device=dev, iterations=5, mask=None).fit(reference, mask="luminosity")      # the same reference; the module's mask is None: the unmasked apply
    ones, zeros = torch.ones(4, 2, device=dev), torch.zeros(4, 2, device=dev)
    assert equal_bits(plain._stain_matrix, norm._stain_matrix) and equal_bits(out, plain.apply(tiles, est, alpha=ones, beta=zeros))
