"""Statistics-space augmentation without a GPU: the new entry points are declared and exported, their argument errors at the C ABI return
before anything is enqueued, the classes validate before any GPU work, the draws follow the restated formulas under a seeded CPU
generator, ``StatisticsDistribution.fit`` and ``ConcentrationStatistics`` compute what they say on hand-made numbers, and the yardstick
of the LAB GPU test (the float32 oracle, tile by tile) stays close to float64 on that test's own tiles and targets."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from oracle import stain_oracle as so
from stainx_amd import (ColorDeconvolution, ColorStatistics, ConcentrationStatistics, Reinhard, StatisticsAugment, StatisticsDistribution, _native, stain_basis,
                        synth)
from tests import _statistics_numpy as sn
from tests import _value_sweep as vs
from tests.test_per_tile_gpu import mixed_batch

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_reinhard_apply_targets": 13, "sx_reinhard_apply_targets_masked": 15, "sx_deconv_moments": 11, "sx_deconv_moments_masked": 12}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
YARDSTICK_CAP = 0.25e-4      # a quarter of the 1e-4 the GPU test holds the kernel to


def distribution(spread: float = 1.0) -> StatisticsDistribution:
    return StatisticsDistribution(torch.tensor([170.0, 150.0, 115.0]), spread * torch.tensor([12.0, 6.0, 5.0]), torch.tensor([40.0, 12.0, 9.0]),
                                  spread * torch.tensor([6.0, 2.0, 1.5]))


def lab_targets() -> tuple[np.ndarray, np.ndarray]:
    """The targets of the LAB GPU test: the per-tile statistics of five synthetic H&E tiles (the CPU oracle's, float32)."""
    tiles = synth.he_batch(5, 96, 96, seed0=700).numpy()
    rows = [so.reinhard_fit(tiles[i:i + 1]) for i in range(5)]
    return np.stack([np.asarray(r[0], np.float32) for r in rows]), np.stack([np.asarray(r[1], np.float32) for r in rows])


# ------------------------------------------------------------------ declarations, exports
def test_declared_exported_and_public():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.ABI_VERSION == 1
    for name in ("StatisticsAugment", "StatisticsDistribution", "ConcentrationStatistics"):
        assert name in stainx_amd.__all__ and hasattr(stainx_amd, name)
    assert ConcentrationStatistics._fields == ("sums", "squares", "pixels")
    assert StatisticsDistribution._fields == ("mean_center", "mean_spread", "std_center", "std_spread")
    assert isinstance(StatisticsAugment(distribution()), torch.nn.Module)


# ------------------------------------------------------------------ C ABI argument errors (nothing is enqueued)
@pytest.mark.parametrize("which", ["product", "diag"])
def test_apply_targets_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32 = _native.DTYPE_CODES[torch.float32]

    def call(images=FAKE, out=FAKE, dtype=f32, n=4, sm=FAKE, ss=FAKE, n_sources=4, tm=FAKE, ts=FAKE, n_targets=4):
        return lib.sx_reinhard_apply_targets(images, out, dtype, n, 64, 64, sm, ss, n_sources, tm, ts, n_targets, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=4, sm=FAKE, ss=FAKE, n_sources=4, tm=FAKE, ts=FAKE, n_targets=4, mask=FAKE, threshold=0.8):
        return lib.sx_reinhard_apply_targets_masked(images, out, dtype, n, 64, 64, sm, ss, n_sources, tm, ts, n_targets, mask, threshold, None)

    for fn in (call, masked):
        for name in ("images", "out", "sm", "ss", "tm", "ts"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        assert fn(n=0) == BAD and fn(n=-2) == BAD
        for rows in (0, 2, 3, 5, -1):
            assert fn(n_sources=rows) == BAD and "n_sources" in _native.last_error(lib), rows
            assert fn(n_targets=rows) == BAD and "n_targets" in _native.last_error(lib), rows
        assert fn(dtype=17) == DTYPE and fn(dtype=17, n_sources=1, n_targets=1) == DTYPE
    for threshold in (0.0, 1.0, -0.5, float("nan")):      # (the rule's threshold matters only without an explicit mask)
        assert masked(mask=None, threshold=threshold) == BAD and "luminosity_threshold" in _native.last_error(lib), threshold
    assert masked(mask=None, threshold=0.8, dtype=17) == DTYPE and masked(threshold=7.0, dtype=17) == DTYPE


@pytest.mark.parametrize("which", ["product", "diag"])
def test_moments_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, cl, classic = _native.DTYPE_CODES[torch.float32], _native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC

    def call(images=FAKE, dtype=f32, n=2, h=8, w=8, basis=FAKE, nb=1, per_tile=1, out=FAKE, flags=0):
        return lib.sx_deconv_moments(images, dtype, n, h, w, basis, nb, per_tile, out, flags, None)

    def masked(mask=FAKE, flags=0, out=FAKE, nb=1, images=FAKE, basis=FAKE):
        return lib.sx_deconv_moments_masked(images, f32, 2, 8, 8, basis, nb, 1, out, mask, flags, None)

    cases = ((lambda: call(images=None), "null"), (lambda: call(basis=None), "null"), (lambda: call(out=None), "out pointer is null"), (lambda: call(n=0), "positive"),
             (lambda: call(h=0), "positive"), (lambda: call(nb=3), "n_bases"), (lambda: call(nb=0), "n_bases"), (lambda: call(n=1 << 20, h=1 << 10, w=1 << 10), "2^32"),
             (lambda: call(flags=_native.MACENKO_NORMALIZE_0_1), "no output image"), (lambda: call(flags=_native.MACENKO_OUT_BF16), "no output image"),
             (lambda: call(flags=_native.MACENKO_OUT_F16), "no output image"), (lambda: call(flags=_native.MACENKO_SAMPLED), "no output image"),
             (lambda: masked(mask=None), "mask pointer is null"), (lambda: masked(flags=cl), "planar"), (lambda: masked(out=None), "out pointer is null"),
             (lambda: masked(images=None), "null"), (lambda: masked(basis=None), "null"), (lambda: masked(nb=3), "n_bases"),
             (lambda: masked(flags=_native.MACENKO_NORMALIZE_0_1), "no output image"))
    for bad_call, what in cases:
        assert bad_call() == BAD and what in _native.last_error(lib), (what, _native.last_error(lib))
    assert call(dtype=99, flags=cl | classic) == DTYPE      # (the two allowed flags pass the flag check; nothing is enqueued for an unknown element type)


# ------------------------------------------------------------------ Python argument errors, all before any GPU work
def test_reinhard_apply_target_errors_come_before_gpu_work():
    r = Reinhard(device="cuda")
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    rows = (torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(ValueError, match="Must call fit"):      # (target=None is the fitted path, as before)
        r.apply(x, rows)
    with pytest.raises(ValueError, match="target must be"):
        r.apply(x, rows, target=torch.zeros(3))
    with pytest.raises(ValueError, match="target mean must have shape"):
        r.apply(x, rows, target=(torch.zeros(2, 3), torch.ones(2, 3)))
    with pytest.raises(ValueError, match="target std must have shape"):
        r.apply(x, rows, target=(torch.zeros(3), torch.ones(4)))
    with pytest.raises(ValueError, match="target mean and std must have the same number of rows"):
        r.apply(x, rows, target=(torch.zeros(4, 3), torch.ones(1, 3)))
    with pytest.raises(ValueError, match="source mean must have shape"):
        r.apply(x, (torch.zeros(2, 3), torch.ones(2, 3)), target=rows)
    with pytest.raises(ValueError, match="expects NCHW"):
        r.apply(x[0], rows, target=rows)
    with pytest.raises(ValueError, match="mask shape"):
        r.apply(x, rows, torch.ones(4, 7, 8, dtype=torch.uint8), target=rows)


def test_estimate_and_match_errors_come_before_gpu_work():
    cd = ColorDeconvolution("hed")
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    rows = (torch.zeros(2, 3), torch.ones(2, 3))
    with pytest.raises(ValueError, match="expects a tensor"):
        cd.estimate(x.numpy())
    with pytest.raises(ValueError, match="expects CHW / NCHW"):
        cd.estimate(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        cd.estimate(x, mask=torch.ones(2, 8, 8))
    with pytest.raises(ValueError, match="planar"):
        ColorDeconvolution("hed", channel_axis=-1).estimate(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), mask="luminosity")
    with pytest.raises(ValueError, match="holds 3 bases for a batch of 2 tiles"):
        ColorDeconvolution(torch.stack([stain_basis("hed")] * 3)).estimate(x)
    with pytest.raises(ValueError, match="runs on a CUDA"):      # everything above came first: only now would the GPU be touched
        cd.estimate(x)
    for bad in ((0.0, 2.5), (2.0, 1.0), (0.1,), "wide", (0.1, float("inf"))):
        with pytest.raises(ValueError, match="gain_range"):
            cd.match(x, rows, rows, gain_range=bad)
    with pytest.raises(ValueError, match="source must be"):
        cd.match(x, torch.zeros(2, 3), rows)
    with pytest.raises(ValueError, match="target mean must be a tensor of shape"):
        cd.match(x, rows, (torch.zeros(3, 3), torch.ones(3, 3)))
    with pytest.raises(ValueError, match="same number of rows"):
        cd.match(x, (torch.zeros(2, 3), torch.ones(1, 3)), rows)
    three = ConcentrationStatistics(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="source holds"):
        cd.match(x, three, rows)
    with pytest.raises(ValueError, match="mask shape"):
        cd.match(x, rows, rows, mask=torch.ones(2, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="runs on a CUDA"):
        cd.match(x, rows, rows)


def test_augment_errors_come_before_gpu_work():
    d = distribution()
    with pytest.raises(ValueError, match="distribution must be"):
        StatisticsAugment((d.mean_center, d.std_center))
    with pytest.raises(ValueError, match="mean_spread must be a tensor of shape"):
        StatisticsAugment(StatisticsDistribution(d.mean_center, torch.zeros(2), d.std_center, d.std_spread))
    for kwargs, what in (({"space": "hsv"}, "space"), ({"kind": "cauchy"}, "kind"), ({"spread_scale": -1.0}, "spread_scale"), ({"spread_scale": float("nan")}, "spread_scale"),
                         ({"p": 1.5}, "p must"), ({"p": -0.1}, "p must"), ({"gain_range": (0.0, 1.0)}, "gain_range"), ({"mask": "otsu"}, "mask must be"),
                         ({"luminosity_threshold": 1.5}, "luminosity_threshold"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            StatisticsAugment(d, **kwargs)
    with pytest.raises(ValueError, match="unknown stain basis"):
        StatisticsAugment(d, "hed", basis="xyz")
    assert StatisticsAugment(d, "lab").deconv is None      # (no deconvolution in the LAB space)
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    for space in ("lab", "hed"):
        aug = StatisticsAugment(d, space)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            aug(torch.zeros(4, 8, 8, 3, dtype=torch.uint8))
        with pytest.raises(ValueError, match="expects a tensor"):
            aug(x.numpy())
        with pytest.raises(ValueError, match="targets must be"):
            aug(x, targets=torch.zeros(4, 3))
        with pytest.raises(ValueError, match="targets std must be a tensor of shape"):
            aug(x, targets=(torch.zeros(4, 3), torch.zeros(3, 3)))
        with pytest.raises(ValueError, match="same number of rows"):
            aug(x, targets=(torch.zeros(4, 3), torch.zeros(1, 3)))
        with pytest.raises(ValueError, match="mask dtype"):
            aug(x, mask=torch.ones(4, 8, 8))
        with pytest.raises(ValueError, match="runs on a CUDA"):      # everything above came first
            aug(x)
    assert "space='hed'" in repr(StatisticsAugment(d, "hed", kind="laplace", p=0.5)) and "kind='laplace'" in repr(StatisticsAugment(d, "hed", kind="laplace", p=0.5))
    with pytest.raises(ValueError, match="needs own="):
        StatisticsAugment(d, p=0.5).sample_targets(4, "cpu")


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("kind", ["normal", "laplace", "uniform"])
def test_sample_targets_follow_the_restated_formulas(kind):
    d, n, scale = distribution(), 37, 0.75
    aug = StatisticsAugment(d, kind=kind, spread_scale=scale, generator=torch.Generator().manual_seed(1234))
    mean, std = aug.sample_targets(n, "cpu")
    again = torch.Generator().manual_seed(1234)
    raw = (torch.randn if kind == "normal" else torch.rand)((2, n, 3), generator=again, dtype=torch.float32).numpy()
    want_mean, want_std = sn.targets_of(kind, raw, [t.numpy() for t in d], scale)
    assert mean.shape == (n, 3) and std.shape == (n, 3) and mean.dtype == torch.float32
    if kind == "laplace":      # (the logarithm is the platform's: z within 3 units in its last place, times the spread, and the sum's own rounding)
        z = np.abs(sn.z_of(kind, raw))
        for got, want, spread, zz in ((mean.numpy(), want_mean, d.mean_spread.numpy(), z[0]), (std.numpy(), want_std, d.std_spread.numpy(), z[1])):
            bound = 3.0 * np.spacing(zz) * np.float32(scale) * spread + np.spacing(np.abs(want))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound).all(), float((np.abs(got - want) / bound).max())
    else:
        assert np.array_equal(mean.numpy(), want_mean) and np.array_equal(std.numpy(), want_std)
    assert float(np.abs(sn.z_of(kind, raw)).max()) > 0.5      # (something was drawn)
    # p < 1: one more draw, rand(n) < p, in that order; a tile that is not chosen gets its own row
    own = (torch.full((n, 3), 3.0), torch.full((n, 3), 0.5))
    some = StatisticsAugment(d, kind=kind, spread_scale=scale, p=0.4, generator=torch.Generator().manual_seed(1234))
    mean_p, std_p = some.sample_targets(n, "cpu", own=own)
    chosen = (torch.rand((n,), generator=again, dtype=torch.float32) < 0.4).numpy()
    assert 0 < chosen.sum() < n
    assert np.array_equal(mean_p.numpy()[chosen], mean.numpy()[chosen]) and np.array_equal(std_p.numpy()[chosen], std.numpy()[chosen])
    assert (mean_p.numpy()[~chosen] == 3.0).all() and (std_p.numpy()[~chosen] == 0.5).all()
    # zero spreads: the centres exactly, whatever was drawn
    for flat in (StatisticsAugment(distribution(0.0), kind=kind), StatisticsAugment(d, kind=kind, spread_scale=0.0)):
        m0, s0 = flat.sample_targets(5, "cpu")
        assert torch.equal(m0, d.mean_center.expand(5, 3)) and torch.equal(s0, d.std_center.expand(5, 3))


def test_the_restated_draws():
    raw = np.array([0.0, 0.25, 0.5, 0.75, 1.0 - 2.0**-24], dtype=np.float32)
    assert sn.z_of("uniform", raw).tolist() == [-1.0, -0.5, 0.0, 0.5, float(np.float32(1.0) - np.float32(2.0**-23))]
    z = sn.z_of("laplace", raw)
    assert z[2] == 0.0 and np.isclose(z[1], np.log(0.5)) and np.isclose(z[3], -np.log(0.5)) and np.isfinite(z).all() and z[0] < -80.0
    assert sn.z_of("normal", raw) is not None and np.array_equal(sn.z_of("normal", raw), raw)


# ------------------------------------------------------------------ StatisticsDistribution.fit
def test_fit_skips_nan_rows_and_refuses_fewer_than_two():
    rng = np.random.default_rng(5)
    means, stds = rng.normal(150.0, 10.0, (7, 3)).astype(np.float32), rng.uniform(5.0, 30.0, (7, 3)).astype(np.float32)
    means[2, 1] = np.nan
    stds[5] = np.nan
    want = sn.fit_distribution(means, stds)
    a = ColorStatistics(torch.from_numpy(means[:4]), torch.from_numpy(stds[:4]))
    b = (torch.from_numpy(means[4:6]), torch.from_numpy(stds[4:6]))
    c = (torch.from_numpy(means[6]), torch.from_numpy(stds[6]))      # a single row, (3,)
    got = StatisticsDistribution.fit(a, b, c)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == (3,) and np.array_equal(g.numpy(), w)
    valid = [0, 1, 3, 4, 6]
    assert np.allclose(got.mean_center.numpy(), means[valid].astype(np.float64).mean(0)) and np.allclose(got.std_spread.numpy(), stds[valid].astype(np.float64).std(0, ddof=1))
    # ConcentrationStatistics enter as (mean(), std()); a set of fewer than two pixels is a NaN row and is skipped
    sums = torch.tensor([[65536 * 10, 0, -65536 * 4], [65536 * 30, 65536 * 6, 0], [5, 5, 5]], dtype=torch.int64)
    squares = torch.tensor([[(1 << 24) * 30, 0, (1 << 24) * 6], [(1 << 24) * 100, (1 << 24) * 9, 0], [1, 1, 1]], dtype=torch.int64)
    cs = ConcentrationStatistics(sums, squares, torch.tensor([10, 10, 1], dtype=torch.int64))
    from_cs = StatisticsDistribution.fit(cs)
    m, s = sn.mean_std(sums.numpy(), squares.numpy(), cs.pixels.numpy())
    for g, w in zip(from_cs, sn.fit_distribution(m, s)):
        assert np.array_equal(g.numpy(), w)
    with pytest.raises(ValueError, match="at least two rows"):
        StatisticsDistribution.fit((torch.from_numpy(means[1:3]), torch.from_numpy(stds[1:3])))
    with pytest.raises(ValueError, match="at least two rows"):
        StatisticsDistribution.fit(c)
    with pytest.raises(ValueError, match="at least one"):
        StatisticsDistribution.fit()
    with pytest.raises(ValueError, match="fit takes"):
        StatisticsDistribution.fit(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="shape"):
        StatisticsDistribution.fit((torch.zeros(4, 2), torch.zeros(4, 2)))
    with pytest.raises(ValueError, match="same number of rows"):
        StatisticsDistribution.fit((torch.zeros(4, 3), torch.zeros(3, 3)))


# ------------------------------------------------------------------ ConcentrationStatistics
def test_concentration_statistics_on_hand_made_integers():
    # stain 0: the values 1, 2, 3, 4 (mean 2.5, unbiased variance 5/3); stain 1: constant 0.5; stain 2: -1, 1
    vals = np.array([[1.0, 2.0, 3.0, 4.0], [0.5, 0.5, 0.5, 0.5], [-1.0, 1.0, -1.0, 1.0]], dtype=np.float32).reshape(1, 3, 2, 2)
    sums, squares, pixels = sn.moments_of(vals)
    assert sums.tolist() == [[10 << 16, 2 << 16, 0]] and squares.tolist() == [[30 << 24, 1 << 24, 4 << 24]] and pixels.tolist() == [4]
    cs = ConcentrationStatistics(torch.from_numpy(sums), torch.from_numpy(squares), torch.from_numpy(pixels))
    assert cs.mean().dtype == torch.float64 and cs.mean().tolist() == [[2.5, 0.5, 0.0]]
    assert torch.allclose(cs.std(), torch.tensor([[np.sqrt(5.0 / 3.0), 0.0, np.sqrt(4.0 / 3.0)]], dtype=torch.float64), rtol=1e-15, atol=0.0)
    m, s = sn.mean_std(sums, squares, pixels)
    assert np.array_equal(cs.mean().numpy(), m) and np.array_equal(cs.std().numpy(), s)
    # fewer than two pixels: NaN, both; the floor on a constant set never gives a negative variance
    few = ConcentrationStatistics(torch.tensor([[7, 7, 7], [0, 0, 0]]), torch.tensor([[0, 0, 0], [0, 0, 0]]), torch.tensor([1, 0]))
    assert torch.isnan(few.mean()).all() and torch.isnan(few.std()).all()
    third = np.full((1, 3, 1, 9), 1.0 / 3.0, dtype=np.float32)
    flat = ConcentrationStatistics(*(torch.from_numpy(v) for v in sn.moments_of(third)))
    assert (flat.std() == 0.0).all() and torch.allclose(flat.mean(), torch.full((1, 3), 1.0 / 3.0, dtype=torch.float64), atol=2.0**-17)
    # pool: exact sums of every set of every argument
    other = ConcentrationStatistics(torch.tensor([[1, 2, 3], [4, 5, 6]]), torch.tensor([[7, 8, 9], [1, 1, 1]]), torch.tensor([2, 3]))
    both = ConcentrationStatistics.pool(cs, other)
    assert both.sums.tolist() == [[(10 << 16) + 5, (2 << 16) + 7, 9]] and both.squares.tolist() == [[(30 << 24) + 8, (1 << 24) + 9, (4 << 24) + 10]] and both.pixels.tolist() == [9]
    assert both.sums.dtype == torch.int64 and tuple(both.pixels.shape) == (1,)
    with pytest.raises(ValueError, match="at least one"):
        ConcentrationStatistics.pool()
    with pytest.raises(ValueError, match="pool takes"):
        ConcentrationStatistics.pool(cs, (cs.sums, cs.squares, cs.pixels))


def test_the_restated_moments_rule():
    c = np.array([0.5 * 2.0**-16, 1.5 * 2.0**-16, 64.0, 65.0, -1e9, 3e38, 2.0**-12], dtype=np.float32)
    t = sn.qn.terms_of(c)
    assert t.tolist() == [0, 2, 1 << 22, 65 << 16, -(2**31), 2**31 - 1, 16]
    assert sn.squares_of(t).tolist() == [0, 0, 1 << 36, 1 << 36, 1 << 36, 1 << 36, 1]      # (clamped at 64; 16 * 16 >> 8)
    assert sn.squares_of(np.array([15, -15, 17])).tolist() == [0, 0, 1]      # floored
    conc = np.zeros((1, 3, 1, 4), np.float32)
    conc[0, :, 0, 0] = 2.0
    conc[0, 1, 0, 2] = np.nan
    conc[0, 0, 0, 3] = np.inf
    sums, squares, px = sn.moments_of(conc, keep=np.array([[[True, False, True, True]]]))
    assert px.tolist() == [1] and sums.tolist() == [[2 << 16] * 3] and squares.tolist() == [[4 << 24] * 3]
    # match: the clamp of the gain, the NaN / zero-std rows
    sm, ss = np.array([[1.0, 2.0, 3.0], [1.0, np.nan, 3.0], [1.0, 2.0, 3.0]], np.float32), np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 0.0, 1.0]], np.float32)
    alpha, beta = sn.match_factors(sm, ss, np.array([0.5, 0.5, 0.5], np.float32), np.array([0.01, 1.5, 9.0], np.float32), 3)
    assert alpha[0].tolist() == [float(np.float32(0.1)), 1.5, 2.5] and np.array_equal(beta[0], np.float32(0.5) - alpha[0] * sm[0])
    assert alpha[1:].tolist() == [[1.0] * 3] * 2 and beta[1:].tolist() == [[0.0] * 3] * 2


def test_match_factors_equal_the_restatement_on_cpu_tensors():
    from stainx_amd.deconv import match_factors

    rng = np.random.default_rng(11)
    sm, ss = rng.normal(0.4, 0.3, (6, 3)).astype(np.float32), rng.uniform(0.01, 0.6, (6, 3)).astype(np.float32)
    tm, ts = rng.normal(0.4, 0.3, (6, 3)).astype(np.float32), rng.uniform(0.01, 0.6, (6, 3)).astype(np.float32)
    sm[1, 0], ss[2, 2], tm[3, 1], ss[4, 1] = np.nan, 0.0, np.nan, np.nan
    for gain in ((0.1, 2.5), (0.5, 1.25)):
        alpha, beta = match_factors(*(torch.from_numpy(v) for v in (sm, ss, tm, ts)), 6, gain)
        want_a, want_b = sn.match_factors(sm, ss, tm, ts, 6, gain)
        assert alpha.dtype == torch.float32 and np.array_equal(alpha.numpy(), want_a) and np.array_equal(beta.numpy(), want_b)
        assert alpha[1:5].eq(1.0).all() and beta[1:5].eq(0.0).all() and not alpha[0].eq(1.0).all()
    alpha, _ = match_factors(torch.from_numpy(sm[0]), torch.from_numpy(ss[0]), torch.from_numpy(tm[:1]), torch.from_numpy(ts[:1]), 6, (0.1, 2.5))
    assert tuple(alpha.shape) == (6, 3) and np.array_equal(alpha.numpy(), sn.match_factors(sm[0], ss[0], tm[:1], ts[:1], 6)[0])


# ------------------------------------------------------------------ the yardstick of the LAB GPU test
def test_the_lab_yardstick_stays_close_to_float64():
    """The float32 oracle (``so.reinhard_transform``, tile by tile, with the target of the tile) against float64 (tests/_value_sweep.py:
    ``reinhard64`` with the oracle's own float32 statistics) on the GPU test's tiles and targets: measured 5.2e-7 here, with ratios of
    target to source standard deviation down to 0.06 on the noise tiles."""
    x = mixed_batch()[0].numpy()
    t_mean, t_std = lab_targets()
    worst, ratios = 0.0, []
    for i in range(x.shape[0]):
        tile = so.to_unit_float(x[i:i + 1])      # (the float32 case of the GPU test)
        got = so.reinhard_transform(tile, t_mean[i], t_std[i])
        mean, std = so.reinhard_fit(tile)
        unit = tile.transpose(0, 2, 3, 1).reshape(-1, 3)
        want = vs.reinhard64(unit, mean, std, t_mean[i], t_std[i])["out"].reshape(1, 96, 96, 3).transpose(0, 3, 1, 2)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        ratios.append(float((np.asarray(t_std[i], np.float64) / np.asarray(std, np.float64)).min()))
    print(f"float32 oracle against float64 on the LAB tiles: max |diff| {worst:.3e}; smallest target / source std per tile {[round(r, 3) for r in ratios]}")
    assert worst <= YARDSTICK_CAP, worst
