"""Tone augmentation without a GPU: the generator's restatement (tests/_tone_numpy.py) gives Random123's known answers and a field with
the moments of independent standard normals, the four entry points are declared and exported, their argument errors at the C ABI return
before anything is enqueued, and ``ToneAugment`` / ``GaussianNoiseAugment`` / ``GreyStatistics`` validate, draw and pool what they say."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import GaussianNoiseAugment, GreyStatistics, ToneAugment, _native, adjust_tone, grey_statistics
from tests import _tone_numpy as tn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_tone_apply": 12, "sx_tone_apply_masked": 13, "sx_grey_statistics": 9, "sx_grey_statistics_masked": 10}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE


# ------------------------------------------------------------------ the generator
def _words(text: str) -> list[int]:
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter, key, words", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, words):
    got = tn.philox4x32_10(np.array(_words(counter), dtype=np.uint64), np.array(_words(key), dtype=np.uint64))
    assert [int(w) for w in got] == _words(words)


def test_field_moments():
    """Seed 1, pixels 0 .. 65535: each of the four normals has the mean, the spread and the independence of a standard normal sample of
    that size (4 standard errors); the generator is deterministic, so the figures are fixed."""
    n = 65536
    z = tn.normals(1, np.arange(n))
    assert z.shape == (n, 4) and np.isfinite(z).all()
    mean, std = np.abs(z.mean(axis=0)), np.abs(z.std(axis=0) - 1.0)
    corr = np.corrcoef(z.T) - np.eye(4)
    print(f"field moments: |mean| <= {mean.max():.4f}, |std - 1| <= {std.max():.4f}, |corr| <= {np.abs(corr).max():.4f}, max |z| = {np.abs(z).max():.3f}")
    assert mean.max() <= 4.0 / math.sqrt(n)
    assert std.max() <= 4.0 / math.sqrt(2.0 * n)
    assert np.abs(corr).max() <= 4.0 / math.sqrt(n)
    assert np.abs(z).max() < math.sqrt(-2.0 * math.log(2.0**-24))
    # the field is a function of (seed, pixel): a subset of the pixels, in another order, gives the same normals; another seed another field
    some = np.array([65535, 7, 4096, 0])
    assert np.array_equal(tn.normals(1, some), z[some])
    assert not np.array_equal(tn.normals(2, some), z[some])
    # a pixel index past 2^32 uses the counter's second word; a seed's upper half the key's second word
    assert not np.array_equal(tn.normals(1, np.array([1 << 32])), tn.normals(1, np.array([0])))
    assert not np.array_equal(tn.normals(1 + (1 << 32), some), z[some])
    assert np.array_equal(tn.normals(-1, some), tn.normals((1 << 64) - 1, some))      # (an int64 seed is its two's-complement words)


def test_uniform_is_exact_in_float32_and_open():
    ends = tn.uniform(np.array([0, 0xFFFFFFFF, 1 << 9, 0x1FF], dtype=np.uint32))
    assert ends.tolist() == [2.0**-24, 1.0 - 2.0**-24, 3.0 * 2.0**-24, 2.0**-24]
    words = np.random.default_rng(3).integers(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32)
    u = tn.uniform(words)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() > 0.0 and u.max() < 1.0
    assert np.float32(ends[0]) > 0.0 and np.float32(ends[1]) < np.float32(1.0)


# ------------------------------------------------------------------ the rule's restatement
def test_restatement_identity_copies_and_steps():
    rng = np.random.default_rng(11)
    levels = rng.integers(0, 256, size=(500, 3)).astype(np.float64)
    out, copied = tn.levels64(levels, tn.IDENTITY)
    assert np.array_equal(out, levels) and not copied.any()
    out, copied = tn.levels64(levels, tn.IDENTITY, seed=5, pixels=np.arange(500))      # sigma == 0 with a seed adds nothing
    assert np.array_equal(out, levels)
    for row in ((float("nan"), 0, 1, 0), (1, float("inf"), 1, 0), (1, 0, 0.0, 0), (1, 0, -1.0, 0), (1, 0, 1, -0.1), (1, 0, float("nan"), 0.1)):
        out, copied = tn.levels64(levels, row, seed=5, pixels=np.arange(500))
        assert copied.all() and np.array_equal(out, levels), row
    odd = np.array([[np.nan, 100.0, 50.0], [10.0, np.inf, 20.0], [300.0, -5.0, 128.0]])
    out, copied = tn.levels64(odd, (0.5, 0.1, 1.0, 0.0))
    assert copied.tolist() == [True, False, False] and out[0].tolist() == [0.0, 100.0, 50.0]
    assert np.allclose(out[1:], [[30.5, 153.0, 35.5], [153.0, 25.5, 89.5]], atol=1e-5)      # (0.1 as a float32)
    out, _ = tn.levels64(np.array([[0.0, 63.75, 255.0]]), (1.0, 0.0, 2.0, 0.0))
    assert np.allclose(out, [[0.0, 63.75**2 / 255.0, 255.0]])
    # noise: t + 255 sigma z of the pixel's normals, per channel or shared
    z = tn.normals(9, np.arange(500))
    mid = np.full((500, 3), 128.0)
    sigma = float(np.float32(0.02))
    out, _ = tn.levels64(mid, (1.0, 0.0, 1.0, 0.02), seed=9, pixels=np.arange(500))
    assert np.allclose(out, 128.0 + 255.0 * sigma * z[:, :3], atol=1e-12)
    out, _ = tn.levels64(mid, (1.0, 0.0, 1.0, 0.02), seed=9, pixels=np.arange(500), shared=True)
    assert np.allclose(out, np.repeat(128.0 + 255.0 * sigma * z[:, 3:4], 3, axis=1), atol=1e-12)


# ------------------------------------------------------------------ the C ABI
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
    for name in ("ToneAugment", "GaussianNoiseAugment", "GreyStatistics", "adjust_tone", "grey_statistics"):
        assert name in stainx_amd.__all__ and hasattr(stainx_amd, name)
    assert isinstance(ToneAugment(), torch.nn.Module) and isinstance(GaussianNoiseAugment(), ToneAugment) and callable(adjust_tone) and callable(grey_statistics)


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, rows=FAKE, n_rows=3, seeds=FAKE, shared=0, flags=0):
        return lib.sx_tone_apply(images, out, dtype, n, h, w, rows, n_rows, seeds, shared, flags, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, rows=FAKE, n_rows=3, seeds=FAKE, shared=0, mask=FAKE, flags=0):
        return lib.sx_tone_apply_masked(images, out, dtype, n, h, w, rows, n_rows, seeds, shared, mask, flags, None)

    for fn in (call, masked):
        for seeds in (FAKE, None):      # (a NULL seeds pointer is "no noise", not an error: the other checks still come first)
            for name in ("images", "out", "rows"):
                assert fn(**{name: None}, seeds=seeds) == BAD and "null" in _native.last_error(lib), name
            for size in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": -1}):
                assert fn(**size, seeds=seeds) == BAD and "positive" in _native.last_error(lib), size
            assert fn(n=1 << 20, h=1 << 10, w=1 << 10, n_rows=1, seeds=seeds) == BAD and "2^32" in _native.last_error(lib)
            for rows in (0, 2, 4, -1):
                assert fn(n_rows=rows, seeds=seeds) == BAD and "n_rows" in _native.last_error(lib), rows
            for flags in (_native.MACENKO_SAMPLED, 1 << 20, _native.MACENKO_TWO_PASS, bf16, f16):      # (the output flags: uint8 input only)
                assert fn(flags=flags, seeds=seeds) == BAD, flags
            assert fn(dtype=u8, flags=bf16 | f16, seeds=seeds) == BAD      # (one of the two)
            assert fn(dtype=17, seeds=seeds) == DTYPE and fn(dtype=17, n_rows=1, flags=classic | unit, shared=1, seeds=seeds) == DTYPE and fn(dtype=-1, seeds=seeds) == DTYPE
    assert call(dtype=99, flags=cl) == DTYPE      # (the unmasked call takes the layout flag; nothing is enqueued for an unknown element type)
    assert masked(mask=None) == BAD and "mask pointer is null" in _native.last_error(lib)
    assert masked(flags=cl) == BAD and "planar" in _native.last_error(lib)
    assert masked(flags=cl, dtype=17) == BAD      # (the argument errors come before the dtype)

    def stats(images=FAKE, dtype=f32, n=3, h=8, w=8, last=0, pooled=0, out=FAKE):
        return lib.sx_grey_statistics(images, dtype, n, h, w, last, pooled, out, None)

    def stats_masked(images=FAKE, dtype=f32, n=3, h=8, w=8, last=0, pooled=0, mask=FAKE, out=FAKE):
        return lib.sx_grey_statistics_masked(images, dtype, n, h, w, last, pooled, mask, out, None)

    for fn in (stats, stats_masked):
        for name in ("images", "out"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        for size in ({"n": 0}, {"h": -3}, {"w": 0}):
            assert fn(**size) == BAD and "positive" in _native.last_error(lib), size
        assert fn(n=1 << 40) == BAD and "too many tiles" in _native.last_error(lib)
        assert fn(dtype=17) == DTYPE and fn(dtype=-1, pooled=1) == DTYPE      # (before the clearing memset)
    assert stats(dtype=17, last=1) == DTYPE
    assert stats_masked(mask=None) == BAD and "mask pointer is null" in _native.last_error(lib)
    assert stats_masked(last=1) == BAD and "planar" in _native.last_error(lib)


# ------------------------------------------------------------------ the modules
def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"brightness": 1.0}, "brightness"), ({"brightness": -0.1}, "brightness"), ({"brightness": float("nan")}, "brightness"), ({"brightness": "wide"}, "brightness"),
                         ({"contrast": 1.0}, "contrast"), ({"contrast": -0.2}, "contrast"), ({"contrast": float("inf")}, "contrast"), ({"shift": -0.1}, "shift"),
                         ({"shift": float("inf")}, "shift"), ({"gamma": -0.1}, "gamma"), ({"gamma": float("nan")}, "gamma"), ({"noise": -1e-3}, "noise"), ({"noise": float("inf")}, "noise"),
                         ({"pivot": "median"}, "pivot"), ({"pivot": 1.5}, "pivot"), ({"pivot": -0.1}, "pivot"), ({"pivot": None}, "pivot"), ({"p": 1.5}, "p must"), ({"p": -0.1}, "p must"),
                         ({"p": float("nan")}, "p must"), ({"mask": "otsu"}, "mask must be"), ({"luminosity_threshold": 1.5}, "luminosity_threshold"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            ToneAugment(**kwargs)
    for kwargs, what in (({"sigma": -0.1}, "sigma"), ({"sigma": (0.2, 0.1)}, "low <= high"), ({"sigma": (0.1, 0.2, 0.3)}, "pair"), ({"sigma": float("nan")}, "sigma"),
                         ({"sigma": (0.0, float("inf"))}, "sigma"), ({"p": 2.0}, "p must"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            GaussianNoiseAugment(**kwargs)
    aug = ToneAugment(0.999, 0.0, shift=2.0, gamma=0.5, noise=0.05, shared_noise=True, pivot=0.25, p=0.0)
    assert (aug.brightness, aug.contrast, aug.shift, aug.gamma, aug.noise, aug.shared_noise, aug.pivot, aug.p) == (0.999, 0.0, 2.0, 0.5, 0.05, True, 0.25, 0.0)
    assert "brightness=0.999" in repr(aug) and "noise=0.05" in repr(aug) and "pivot=0.25" in repr(aug) and "normalize_to_0_1=True" in repr(aug)
    noise = GaussianNoiseAugment(0.05)
    assert noise.sigma == (0.0, 0.05) and (noise.brightness, noise.contrast, noise.shift, noise.gamma, noise.noise, noise.pivot) == (0.0, 0.0, 0.0, 0.0, 0.05, 0.5)
    assert GaussianNoiseAugment().sigma == (0.0, 0.1) and ToneAugment().pivot == "mean"


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    rows = torch.tensor([tn.IDENTITY] * 4)
    seeds = torch.arange(4, dtype=torch.int64)
    aug = ToneAugment(pivot=0.5)
    for fn in (lambda img, r, **k: adjust_tone(img, r, **k), lambda img, r, **k: aug(img, r, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), rows)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), rows)
        for wrong in (torch.zeros(4, 5), torch.zeros(3, 4), torch.zeros(4, 1), [1.0, 0.0, 1.0, 0.0]):
            with pytest.raises(ValueError, match="rows must be"):
                fn(x, wrong)
        for wrong in (torch.zeros(4), torch.arange(3, dtype=torch.int64), torch.zeros(4, 1, dtype=torch.int64), torch.arange(4, dtype=torch.int32), [1, 2, 3, 4]):
            with pytest.raises(ValueError, match="seeds must be"):
                fn(x, rows, seeds=wrong)
        with pytest.raises(ValueError, match="mask dtype"):
            fn(x, rows, seeds=seeds, mask=torch.ones(4, 8, 8))
        with pytest.raises(ValueError, match="mask shape"):
            fn(x, rows, mask=torch.ones(4, 8, 9, dtype=torch.uint8))
        with pytest.raises(ValueError, match="runs on a CUDA"):      # everything above came first: only now would the GPU be touched
            fn(x, rows, seeds=seeds)
    with pytest.raises(ValueError, match="channel_axis"):
        adjust_tone(x, rows, channel_axis=2)
    with pytest.raises(ValueError, match="planar"):
        adjust_tone(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), rows, channel_axis=-1, mask="luminosity")
    with pytest.raises(ValueError, match="luminosity_threshold"):
        adjust_tone(x, rows, luminosity_threshold=0.0)
    # grey_statistics
    with pytest.raises(ValueError, match="4-D image tensor"):
        grey_statistics(x[0])
    with pytest.raises(ValueError, match="3 channels"):
        grey_statistics(torch.zeros(4, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channel_axis"):
        grey_statistics(x, channel_axis=2)
    with pytest.raises(ValueError, match="luminosity_threshold"):
        grey_statistics(x, luminosity_threshold=1.0)
    with pytest.raises(ValueError, match="mask shape"):
        grey_statistics(x, mask=torch.ones(4, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="planar"):
        grey_statistics(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), channel_axis=-1, mask="luminosity")
    with pytest.raises(ValueError, match="runs on a CUDA"):
        grey_statistics(x)
    with pytest.raises(ValueError, match="grey means"):
        ToneAugment().sample_rows(4, None, "cpu")
    with pytest.raises(ValueError, match="means must be"):
        ToneAugment().sample_rows(4, torch.zeros(3), "cpu")


def test_sample_rows_and_seeds():
    n = 4000
    make = lambda **k: ToneAugment(0.2, 0.3, shift=0.05, gamma=0.4, noise=0.08, generator=torch.Generator().manual_seed(77), **k)      # noqa: E731
    means = torch.linspace(40.0, 220.0, n, dtype=torch.float64)
    rows = make().sample_rows(n, means, "cpu")
    assert tuple(rows.shape) == (n, 4) and rows.dtype == torch.float32 and bool(torch.isfinite(rows).all())
    # the restated draw and the stated order: rand((n, 5)), then rand(n) < p, then randint for the seeds
    again = torch.Generator().manual_seed(77)
    u = torch.rand((n, 5), generator=again, dtype=torch.float32)
    centre, reach = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.04]), torch.tensor([0.2, 0.3, 0.05, 0.4, 0.04])
    r, c, d, log_gamma, sigma = (centre + reach * (2.0 * u - 1.0)).unbind(dim=1)
    want = torch.stack([c * r, (1.0 - c) * r * (means.float() / 255.0) + d, torch.exp(log_gamma), sigma.clamp_min(0.0)], dim=1)
    assert torch.equal(rows, want)
    assert bool((r >= 0.8 - 1e-6).all() and (r <= 1.2 + 1e-6).all() and (c >= 0.7 - 1e-6).all() and (c <= 1.3 + 1e-6).all())
    assert bool((rows[:, 2] >= math.exp(-0.4) - 1e-6).all() and (rows[:, 2] <= math.exp(0.4) + 1e-6).all() and (rows[:, 3] >= 0.0).all() and (rows[:, 3] <= 0.08 + 1e-7).all())
    assert abs(float(rows[:, 3].mean()) - 0.04) <= 4.0 * 0.08 / math.sqrt(12.0 * n)      # 4 standard errors of U[0, 0.08]
    some = make(p=0.3)
    rows_p = some.sample_rows(n, means, "cpu")
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.3
    assert torch.equal(torch.isnan(rows_p).all(dim=1), ~chosen) and torch.equal(rows_p[chosen], rows[chosen])
    seeds = some.sample_seeds(n, "cpu")
    assert seeds.dtype == torch.int64 and tuple(seeds.shape) == (n,) and bool((seeds >= 0).all()) and len(set(seeds.tolist())) == n
    assert torch.equal(seeds, torch.randint(0, 2**63 - 1, (n,), generator=again, dtype=torch.int64))
    # a numeric pivot needs no means: m = 255 pivot
    fixed = make(pivot=0.5).sample_rows(n, None, "cpu")
    assert torch.equal(fixed, torch.stack([c * r, (1.0 - c) * r * 0.5 + d, torch.exp(log_gamma), sigma.clamp_min(0.0)], dim=1))
    # every magnitude 0: the identity row exactly, whatever was drawn and whatever the pivot
    identity = torch.tensor(tn.IDENTITY).expand(7, 4)
    assert torch.equal(ToneAugment(0.0, 0.0).sample_rows(7, torch.linspace(0.0, 255.0, 7), "cpu"), identity)
    assert torch.equal(ToneAugment(0.0, 0.0, pivot=0.3).sample_rows(7, None, "cpu"), identity)
    # a tile with no counted pixel (a NaN mean) gets a NaN row; p = 0: every row is NaN
    holes = ToneAugment(0.0, 0.0).sample_rows(3, torch.tensor([10.0, float("nan"), 30.0]), "cpu")
    assert torch.isnan(holes[1]).any() and torch.equal(holes[[0, 2]], identity[:2])
    assert bool(torch.isnan(ToneAugment(p=0.0, pivot=0.5).sample_rows(9, None, "cpu")).all())
    # the noise-only module: sigma in [low, high], everything else the identity
    noise = GaussianNoiseAugment((0.02, 0.1), generator=torch.Generator().manual_seed(5)).sample_rows(n, None, "cpu")
    assert torch.equal(noise[:, :3], torch.tensor(tn.IDENTITY[:3]).expand(n, 3))
    assert bool((noise[:, 3] >= 0.02 - 1e-7).all() and (noise[:, 3] <= 0.1 + 1e-7).all()) and float(noise[:, 3].max() - noise[:, 3].min()) > 0.07


def test_grey_statistics_pool_adds_exactly_and_scores():
    a = GreyStatistics(torch.tensor([4, 0, 1 << 40]), torch.tensor([400, 0, 3 << 40]), torch.tensor([50000, 0, (1 << 62) - 5]))
    b = GreyStatistics(torch.tensor([6, 0, 1]), torch.tensor([100, 0, 2]), torch.tensor([2500, 0, 4]))
    pooled = GreyStatistics.pool(a, b)
    assert pooled.pixels.tolist() == [10, 0, (1 << 40) + 1] and pooled.sum.tolist() == [500, 0, (3 << 40) + 2] and pooled.sum_squares.tolist() == [52500, 0, (1 << 62) - 1]
    assert all(word.dtype == torch.int64 for word in pooled)
    assert torch.equal(GreyStatistics.pool(a).pixels, a.pixels)
    mean, rms = pooled.mean(), pooled.rms_contrast()
    assert mean.dtype == torch.float64 and mean[0].item() == 50.0 and math.isnan(mean[1].item())
    assert rms[0].item() == math.sqrt(5250.0 - 2500.0) and math.isnan(rms[1].item())
    with pytest.raises(ValueError, match="at least one"):
        GreyStatistics.pool()
    with pytest.raises(ValueError, match="equal shapes"):
        GreyStatistics.pool(a, GreyStatistics(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match="takes GreyStatistics"):
        GreyStatistics.pool(a, (a.pixels, a.sum, a.sum_squares))
