"""Stain quantification without a GPU: the figures of ``StainHistograms`` on hand-made CPU tensors against brute force, the argument
errors of ``ColorDeconvolution.quantify`` (raised before any GPU work), the C ABI's declarations and argument errors, and the input
condition of the float64 GPU test (tests/test_quantify_gpu.py): on the committed real crops few float64 concentrations lie so close to a
bin edge that float32 may put them on the other side."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import ColorDeconvolution, StainHistograms, _native, stain_basis
from tests import _masked_numpy as mn
from tests import _quantify_numpy as qn

NAMES = ("hed", "he", "hdab")
NEAR_EDGE_CAP = 0.02      # per tile and stain, k = 5: a condition on the inputs of the float64 GPU test, not a tolerance of the kernel
FAKE = 1 << 40            # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE


def made_up(k: int = 5, z: int = 64, n: int = 3, pixels: int = 5000, seed: int = 7) -> tuple[np.ndarray, StainHistograms]:
    """Random float32 concentrations (N, 3, 1, P) -- most inside [-2, 6), some beyond either end -- and their histograms by the yardstick."""
    rng = np.random.default_rng(seed)
    conc = (rng.gamma(2.0, 0.6, size=(n, 3, 1, pixels)) - 0.4).astype(np.float32)
    conc[:, :, :, ::97] = -3.5
    conc[:, :, :, 5::131] = 7.25
    counts, sums, px = qn.histogram_of(conc, k, z)
    return conc, StainHistograms(torch.from_numpy(counts), torch.from_numpy(sums), torch.from_numpy(px), k, z)


def test_the_type_is_public():
    assert stainx_amd.StainHistograms is StainHistograms and "StainHistograms" in stainx_amd.__all__
    h = StainHistograms(torch.zeros(1, 3, 256, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    assert (h.bin_log2, h.zero_bin) == (5, 64) and h._fields == ("counts", "sums", "pixels", "bin_log2", "zero_bin")
    edges = h.edges()
    assert edges.dtype == torch.float64 and edges.shape == (257,) and float(edges[0]) == -2.0 and float(edges[64]) == 0.0 and float(edges[256]) == 6.0
    assert float(edges[65] - edges[64]) == 1.0 / 32.0
    assert torch.equal(StainHistograms(h.counts, h.sums, h.pixels, 8, 32).edges(), (torch.arange(257, dtype=torch.float64) - 32) / 256.0)


def test_the_yardstick_bins_by_the_contract():
    c = np.array([-2.0, -2.0 - 2.0**-20, -1e30, 0.0, -(2.0**-30), 1.0 / 32, np.nextafter(np.float32(1.0 / 32), np.float32(0)), 5.99, 6.0, 3e38], dtype=np.float32)
    assert qn.bins_of(c, 5, 64).tolist() == [0, 0, 0, 64, 63, 65, 64, 255, 255, 255]
    assert qn.bins_of(np.array([0.3, -0.3], np.float32), 0, 0).tolist() == [0, 0] and qn.bins_of(np.array([0.999, 1.0], np.float32), 8, 0).tolist() == [255, 255]
    t = np.array([0.5 * 2.0**-16, 1.5 * 2.0**-16, -0.5 * 2.0**-16, 1.0, 3e38, -3e38, 32768.0], dtype=np.float32)
    assert qn.terms_of(t).tolist() == [0, 2, 0, 65536, 2**31 - 1, -(2**31), 2**31 - 1]      # round to nearest even, saturating
    conc = np.zeros((1, 3, 1, 4), np.float32)
    conc[0, 1, 0, 2] = np.nan
    conc[0, 0, 0, 3] = np.inf
    counts, sums, px = qn.histogram_of(conc, 5, 64, keep=np.array([[[True, False, True, True]]]))
    assert px.tolist() == [1] and counts[0, :, 64].tolist() == [1, 1, 1] and counts.sum() == 3 and sums.tolist() == [[0, 0, 0]]


def test_pool_adds_sets_exactly_and_refuses_differing_binning():
    conc, h = made_up()
    _, other = made_up(seed=8, n=2)
    both = StainHistograms.pool(h, other)
    assert both.counts.shape == (1, 3, 256) and both.sums.shape == (1, 3) and both.pixels.shape == (1,) and (both.bin_log2, both.zero_bin) == (5, 64)
    assert torch.equal(both.counts[0], h.counts.sum(0) + other.counts.sum(0)) and torch.equal(both.sums[0], h.sums.sum(0) + other.sums.sum(0))
    assert int(both.pixels[0]) == int(h.pixels.sum() + other.pixels.sum())
    assert torch.equal(StainHistograms.pool(h).counts, h.counts.sum(0, keepdim=True))
    _, fine = made_up(k=8, z=32)
    with pytest.raises(ValueError, match="binned differently"):
        StainHistograms.pool(h, fine)
    with pytest.raises(ValueError, match="binned differently"):
        StainHistograms.pool(h, StainHistograms(h.counts, h.sums, h.pixels, 5, 63))
    with pytest.raises(ValueError, match="at least one"):
        StainHistograms.pool()
    with pytest.raises(ValueError, match="takes StainHistograms"):
        StainHistograms.pool(h, (h.counts, h.pixels))


def test_mean_is_the_fixed_point_sum_over_the_counted_pixels():
    conc, h = made_up()
    mean = h.mean()
    assert mean.dtype == torch.float64 and mean.shape == (3, 3)
    want = conc.astype(np.float64).reshape(3, 3, -1).mean(axis=-1)
    # (each term is rounded to 2^-16: half a unit per pixel at most)
    assert np.abs(mean.numpy() - want).max() <= 2.0**-17
    exact = qn.terms_of(conc).reshape(3, 3, -1).sum(-1) / 65536.0 / conc.shape[-1]
    np.testing.assert_allclose(mean.numpy(), exact, rtol=0, atol=1e-15)


@pytest.mark.parametrize("k,z", [(5, 64), (8, 32), (0, 3)])
def test_figures_against_brute_force(k, z):
    conc, h = made_up(k, z)
    width = 2.0**-k
    thresholds = [(1 - z) * width, 0.0 if 1 <= z <= 255 else width, 8 * width, (255 - z) * width]
    for s in range(3):
        for i in range(conc.shape[0]):
            v = conc[i, s].ravel()
            for t in thresholds:
                assert float(h.positive_fraction(s, t)[i]) == qn.positive_fraction(v, t), (s, i, t)
            for q in (0.0, 0.001, 0.25, 0.5, 0.9, 0.999, 1.0):
                assert float(h.quantile(s, q)[i]) == qn.quantile_edge(v, q, k, z), (s, i, q)
        trio = (width, 4 * width, 16 * width) if z + 16 <= 255 else (width, 2 * width, 3 * width)
        got = h.h_score(s, trio)
        assert got.dtype == torch.float64 and got.shape == (3,)
        for i in range(conc.shape[0]):
            want = qn.h_score(conc[i, s].ravel(), trio)
            assert abs(float(got[i]) - want) <= 1e-12 and 0.0 <= float(got[i]) <= 300.0, (s, i)
    assert float(h.h_score(0, (width, width, width))[0]) == pytest.approx(300.0 * qn.positive_fraction(conc[0, 0].ravel(), width), abs=1e-12)


def test_a_threshold_off_the_edges_is_refused_with_the_nearest_edges():
    _, h = made_up()
    with pytest.raises(ValueError, match=r"not a bin edge.*nearest edges are 0\.15625 and 0\.1875"):
        h.positive_fraction(1, 0.17)
    for t in (-2.0, 6.0, 6.5, -7.0, float("nan"), float("inf")):      # the outer edges: the end bins also hold what lies beyond them
        with pytest.raises(ValueError, match="not a bin edge inside the range"):
            h.positive_fraction(0, t)
    assert h.positive_fraction(0, -2.0 + 1 / 32).shape == (3,) and h.positive_fraction(0, 6.0 - 1 / 32).shape == (3,)
    with pytest.raises(ValueError, match=r"thresholds\[1\].*not a bin edge"):
        h.h_score(1, (0.125, 0.3, 0.5))
    with pytest.raises(ValueError, match="ascending"):
        h.h_score(1, (0.5, 0.25, 0.75))
    with pytest.raises(ValueError, match="three ascending"):
        h.h_score(1, (0.25, 0.5))
    for bad in (3, -1, 1.0, True, "dab"):
        with pytest.raises(ValueError, match="stain must be 0, 1 or 2"):
            h.positive_fraction(bad, 0.25)
    for bad in (-0.1, 1.1, float("nan"), "median"):
        with pytest.raises(ValueError, match="q must"):
            h.quantile(0, bad)


def test_rows_that_counted_nothing():
    _, h = made_up(n=2)
    counts, sums, pixels = h.counts.clone(), h.sums.clone(), h.pixels.clone()
    counts[1], sums[1], pixels[1] = 0, 0, 0
    e = StainHistograms(counts, sums, pixels, 5, 64)
    assert e.mean()[1].tolist() == [0.0, 0.0, 0.0] and float(e.positive_fraction(1, 0.25)[1]) == 0.0 and float(e.h_score(1, (0.25, 0.5, 1.0))[1]) == 0.0
    assert bool(torch.isnan(e.quantile(1, 0.5)[1])) and not bool(torch.isnan(e.quantile(1, 0.5)[0]))
    assert torch.equal(e.mean()[0], h.mean()[0]) and float(e.positive_fraction(1, 0.25)[0]) == float(h.positive_fraction(1, 0.25)[0])


def test_quantify_raises_argument_errors_before_any_gpu_work():
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    cd = ColorDeconvolution("hdab")
    for bad in (-1, 9, 5.0, True, None):
        with pytest.raises(ValueError, match="bin_log2 must be an integer in"):
            cd.quantify(x, bin_log2=bad)
    for bad in (-1, 256, 64.0, None):
        with pytest.raises(ValueError, match="zero_bin must be an integer in"):
            cd.quantify(x, zero_bin=bad)
    with pytest.raises(ValueError, match="mask shape must be"):
        cd.quantify(x, mask=torch.ones(2, 8, 7, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask dtype must be"):
        cd.quantify(x, mask=torch.ones(2, 8, 8))
    last = ColorDeconvolution("hdab", channel_axis=-1)
    with pytest.raises(ValueError, match="planar"):
        last.quantify(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), mask=torch.ones(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="planar"):
        last.quantify(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), mask="luminosity")
    with pytest.raises(ValueError, match="expects HWC / NHWC"):
        last.quantify(x)
    with pytest.raises(ValueError, match="holds 3 bases for a batch of 2 tiles"):
        ColorDeconvolution(torch.stack([stain_basis("hed")] * 3)).quantify(x)
    with pytest.raises(ValueError, match="expects a tensor"):
        cd.quantify(x.numpy())
    with pytest.raises(ValueError, match="runs on a CUDA"):      # everything above came first: only now would the GPU be touched
        cd.quantify(x)


def test_c_abi_declarations_and_argument_errors():
    assert len(_native.SIGNATURES["sx_deconv_quantify"][1]) == 13 and len(_native.SIGNATURES["sx_deconv_quantify_masked"][1]) == 14
    f32, cl, classic = _native.DTYPE_CODES[torch.float32], _native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC

    for lib in (_native.require(), _native.require_diag()):
        _check_calls(lib, f32, cl, classic)


def _check_calls(lib, f32, cl, classic):
    def call(images=FAKE, dtype=f32, n=2, h=8, w=8, basis=FAKE, nb=1, k=5, z=64, per_tile=1, out=FAKE, flags=0):
        return lib.sx_deconv_quantify(images, dtype, n, h, w, basis, nb, k, z, per_tile, out, flags, None)

    def masked(mask=FAKE, flags=0, out=FAKE, k=5):
        return lib.sx_deconv_quantify_masked(FAKE, f32, 2, 8, 8, FAKE, 1, k, 64, 1, out, mask, flags, None)

    cases = ((lambda: call(images=None), "null"), (lambda: call(basis=None), "null"), (lambda: call(out=None), "out pointer is null"), (lambda: call(n=0), "positive"),
             (lambda: call(nb=3), "n_bases"), (lambda: call(k=-1), "bin_log2"), (lambda: call(k=9), "bin_log2"), (lambda: call(z=-1), "zero_bin"), (lambda: call(z=256), "zero_bin"),
             (lambda: call(flags=_native.MACENKO_NORMALIZE_0_1), "no output image"), (lambda: call(flags=_native.MACENKO_OUT_BF16), "no output image"),
             (lambda: masked(mask=None), "mask pointer is null"), (lambda: masked(flags=cl), "planar"), (lambda: masked(out=None), "out pointer is null"),
             (lambda: masked(k=9), "bin_log2"))
    for bad_call, what in cases:
        assert bad_call() == BAD and what in _native.last_error(lib), (what, _native.last_error(lib))
    assert call(dtype=99, flags=cl | classic) == DTYPE      # (the two allowed flags pass the flag check; nothing is enqueued for an unknown element type)


@pytest.mark.parametrize("name", NAMES)
def test_input_condition_of_the_float64_gpu_test(name):
    """Real crops, k = 5: the share of float64 concentrations within CONC_TOL of a bin edge, per tile and stain -- those may land in the
    neighbouring bin in float32, every other value's bin is certain."""
    x = mn.real_crops(256).numpy()
    share = qn.near_edge_share(qn.concentrations64(x, stain_basis(name).numpy()), 5)
    print(f"{name}: near-edge share per tile and stain, max {share.max():.4f} (cap {NEAR_EDGE_CAP})")
    assert share.shape == (6, 3) and share.max() <= NEAR_EDGE_CAP, (name, share)
