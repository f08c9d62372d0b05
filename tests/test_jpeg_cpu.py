"""The JPEG round trip without a GPU: the two entry points are declared and exported, their argument errors at the C ABI return before
anything is enqueued, the numpy restatement of the rule (tests/_jpeg_numpy.py) equals Pillow's bytes -- the committed fixture
tests/golden/jpeg_pillow.npz everywhere, a live Pillow where it is installed --, the table rule is held to hand-written values, and
``jpeg_compress`` / ``JPEGAugment`` validate and draw what they say."""
from __future__ import annotations

import ctypes
import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import JPEGAugment, _native, jpeg_compress
from tests import _jpeg_numpy as jn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_jpeg_roundtrip": 11, "sx_jpeg_roundtrip_masked": 12}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
FIXTURE_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (8, 8), (9, 17), (16, 16), (17, 9), (33, 31), (65, 130))


def test_declared_exported_and_public():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    for name in ("JPEGAugment", "jpeg_compress"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.jpeg, name)
    assert isinstance(JPEGAugment(), torch.nn.Module) and callable(jpeg_compress)
    block = (ROOT / "stainx_amd" / "csrc" / "jpeg_block.hpp").read_text()
    for constant in (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172):      # the twelve constants of the two transforms
        assert str(constant) in block and str(constant) in header, constant
    assert "hip/" not in block      # (no HIP dependency: tools/jpeg_block_check.cpp compiles it for the host)


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, qualities=FAKE, n_rows=3, subsampling=2, flags=0):
        return lib.sx_jpeg_roundtrip(images, out, dtype, n, h, w, qualities, n_rows, subsampling, flags, None)

    def masked(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, qualities=FAKE, n_rows=3, subsampling=2, mask=FAKE, flags=0):
        return lib.sx_jpeg_roundtrip_masked(images, out, dtype, n, h, w, qualities, n_rows, subsampling, mask, flags, None)

    for fn in (call, masked):
        for name in ("images", "out", "qualities"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        for size in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": -1}):
            assert fn(**size) == BAD and "positive" in _native.last_error(lib), size
        assert fn(n=1 << 20, h=1 << 10, w=1 << 10, n_rows=1) == BAD and "2^32" in _native.last_error(lib)
        for rows in (0, 2, 4, -1):
            assert fn(n_rows=rows) == BAD and "n_rows" in _native.last_error(lib), rows
        for sub in (1, 3, -1, 420):
            assert fn(subsampling=sub) == BAD and "subsampling" in _native.last_error(lib), sub
            assert fn(subsampling=sub, dtype=17) == BAD      # (the argument errors come before the dtype)
        for flags in (_native.MACENKO_SAMPLED, 1 << 20, _native.MACENKO_TWO_PASS, bf16, f16):      # (the output flags: uint8 input only)
            assert fn(flags=flags) == BAD, flags
        assert fn(dtype=u8, flags=bf16 | f16) == BAD      # (one of the two)
        for sub in (0, 2):
            assert fn(dtype=17, subsampling=sub) == DTYPE and fn(dtype=17, n_rows=1, flags=classic | unit, subsampling=sub) == DTYPE and fn(dtype=-1, subsampling=sub) == DTYPE
    assert call(dtype=99, flags=cl) == DTYPE      # (the unmasked call takes the layout flag; nothing is enqueued for an unknown element type)
    assert masked(mask=None) == BAD and "mask pointer is null" in _native.last_error(lib)
    assert masked(flags=cl) == BAD and "planar" in _native.last_error(lib)
    assert masked(flags=cl, dtype=17) == BAD      # (the argument errors come before the dtype)


# ------------------------------------------------------------------ the restatement against Pillow
def test_restatement_equals_the_committed_pillow_bytes():
    fixture = np.load(ROOT / "tests" / "golden" / "jpeg_pillow.npz")
    compared = 0
    for h, w in FIXTURE_SHAPES:
        tile = fixture[f"in_{h}x{w}"]
        assert tile.shape == (3, h, w) and tile.dtype == np.uint8
        for q in (1, 35, 75, 100):
            for s in (0, 2):
                assert np.array_equal(jn.roundtrip_levels(tile, q, s), fixture[f"out_{h}x{w}_q{q}_s{s}"]), (h, w, q, s)
                compared += 1
    real = fixture["in_real"]
    assert real.shape == (3, 128, 128)
    for q in (50, 90):
        for s in (0, 2):
            want = fixture[f"out_real_q{q}_s{s}"]
            assert np.array_equal(jn.roundtrip_levels(real, q, s), want), (q, s)
            assert not np.array_equal(want, real)      # a real perturbation
            compared += 1
    assert compared == 92


def test_restatement_equals_a_live_pillow_on_every_small_shape():
    """Every H and W in 1..19 at qualities 35 and 90, both subsamplings -- the narrow 4:2:0 tiles (W <= 4, where libjpeg replicates the
    chroma instead of filtering it) included: none is left out."""
    image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2026)
    for h in range(1, 20):
        for w in range(1, 20):
            tile = rng.integers(0, 256, size=(3, h, w), dtype=np.uint8)
            for q in (35, 90):
                for s in (0, 2):
                    buffer = io.BytesIO()
                    image.fromarray(np.ascontiguousarray(tile.transpose(1, 2, 0)), "RGB").save(buffer, "JPEG", quality=q, subsampling=s)
                    buffer.seek(0)
                    want = np.asarray(image.open(buffer).convert("RGB")).transpose(2, 0, 1)
                    assert np.array_equal(jn.roundtrip_levels(tile, q, s), want), (h, w, q, s)


def test_table_rule_against_hand_written_values():
    luma, chroma = jn.tables(1)      # scale 5000: every entry saturates at 255
    assert (luma == 255).all() and (chroma == 255).all()
    luma, chroma = jn.tables(49)      # scale 5000 // 49 = 102
    assert luma[0].tolist() == [16, 11, 10, 16, 24, 41, 52, 62] and luma[7, 7] == 101 and chroma[0].tolist() == [17, 18, 24, 48, 101, 101, 101, 101]
    luma, chroma = jn.tables(50)      # scale 100: Annex K itself
    assert np.array_equal(luma, jn.LUMINANCE) and np.array_equal(chroma, jn.CHROMINANCE)
    assert luma[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and chroma[3].tolist() == [47, 66, 99, 99, 99, 99, 99, 99]
    luma, chroma = jn.tables(100)      # scale 0: all ones, not zeros
    assert (luma == 1).all() and (chroma == 1).all()
    assert all(np.array_equal(a, b) for a, b in zip(jn.tables(150), jn.tables(100))) and all(np.array_equal(a, b) for a, b in zip(jn.tables(75.9), jn.tables(75)))
    assert jn.tables(75)[0][0].tolist() == [8, 6, 5, 8, 12, 20, 26, 31] and jn.tables(10)[0][0, :4].tolist() == [80, 55, 50, 80]


def test_a_constant_tile_comes_back_constant():
    for level in ((0, 0, 0), (255, 255, 255), (128, 128, 128), (200, 30, 90), (1, 254, 17)):
        tile = np.empty((3, 21, 37), dtype=np.uint8)
        tile[:] = np.array(level, dtype=np.uint8)[:, None, None]
        for q in (1, 50, 100):
            for s in (0, 2):
                got = jn.roundtrip_levels(tile, q, s)
                assert (got == got[:, :1, :1]).all(), (level, q, s)      # (only the DC coefficient is non-zero, in every block alike)


def test_levels_of_float_tiles_and_copied_tiles():
    x = np.array([0.0, 0.49 / 255, 0.51 / 255, 1.5 / 255, 2.5 / 255, 1.0, 1.7, -0.2, np.nan, np.inf, -np.inf], dtype=np.float32)
    assert jn.levels_of(x).tolist() == [0, 0, 1, 2, 2, 255, 255, 0, 0, 255, 0]      # rint: ties to even; a NaN is level 0
    assert jn.levels_of(np.array([3, 250], dtype=np.uint8)).tolist() == [3, 250]
    rng = np.random.default_rng(3)
    tiles = rng.integers(0, 256, size=(6, 3, 9, 11), dtype=np.uint8)
    got = jn.roundtrip(tiles, [50, np.nan, np.inf, 0, -3, 0.5], "444")
    assert np.array_equal(got[1:], tiles[1:]) and not np.array_equal(got[0], tiles[0])
    assert np.array_equal(jn.roundtrip(tiles[:1], 150, 2), jn.roundtrip(tiles[:1], 100, 2)) and not np.array_equal(jn.roundtrip(tiles[:1], 100, 0), tiles[:1])      # 100 is not the identity


# ------------------------------------------------------------------ the module and the functional form
def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"quality": 50}, "pair"), ({"quality": (50,)}, "pair"), ({"quality": (1, 2, 3)}, "pair"), ({"quality": (0, 50)}, "quality lo"),
                         ({"quality": (1, 101)}, "quality hi"), ({"quality": (30.0, 95)}, "quality lo must be an int"), ({"quality": (30, True)}, "quality hi"),
                         ({"quality": ("a", 50)}, "quality lo must be an int"), ({"quality": (60, 50)}, "lo <= hi"), ({"subsampling": "422"}, "subsampling must be one of"),
                         ({"subsampling": 1}, "subsampling"), ({"subsampling": True}, "subsampling"), ({"subsampling": None}, "subsampling"), ({"p": 1.5}, "p must"), ({"p": -0.1}, "p must"),
                         ({"p": float("nan")}, "p must"), ({"mask": "otsu"}, "mask must be"), ({"luminosity_threshold": 1.5}, "luminosity_threshold"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            JPEGAugment(**kwargs)
    aug = JPEGAugment((1, 100), subsampling="444", p=0.0)      # the closed ends
    assert aug.quality == (1, 100) and aug.subsampling == 0 and aug.p == 0.0 and JPEGAugment().quality == (30, 95) and JPEGAugment().subsampling == 2 and JPEGAugment([7, 7], subsampling=2).quality == (7, 7)
    assert "quality=(1, 100)" in repr(aug) and "subsampling=0" in repr(aug) and "p=0.0" in repr(aug) and "normalize_to_0_1=True" in repr(aug) and "mask=None" in repr(aug)
    assert "'luminosity' (luminosity_threshold=0.7)" in repr(JPEGAugment(mask="luminosity", luminosity_threshold=0.7))


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    qualities = torch.full((4,), 50.0)
    aug = JPEGAugment()
    for fn in (lambda *a, **k: jpeg_compress(*a, **k), lambda img, r, **k: aug(img, r, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), qualities)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), qualities)
        for wrong in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(1, 4), torch.zeros(2)):
            with pytest.raises(ValueError, match=r"quality must be an int or a tensor of shape \(\), \(1,\) or \(N,\) = \(4,\)"):
                fn(x, wrong)
        for wrong in (0, 101, -5, 50.0, float("nan"), True, "high", [50, 60]):
            with pytest.raises(ValueError, match=r"quality must be an int in 1\.\.100"):
                fn(x, wrong)
        with pytest.raises(ValueError, match="mask dtype"):
            fn(x, qualities, mask=torch.ones(4, 8, 8))
        with pytest.raises(ValueError, match="mask shape"):
            fn(x, qualities, mask=torch.ones(4, 8, 9, dtype=torch.uint8))
        for fine in (qualities, qualities[:1], torch.tensor(50.0), 1, 50, 100):      # everything above came first: only now would the GPU be touched
            with pytest.raises(ValueError, match="runs on a CUDA"):
                fn(x, fine)
        with pytest.raises(ValueError, match="runs on a CUDA"):      # a CHW tile: N = 1
            fn(x[0], torch.ones(1))
    with pytest.raises(ValueError, match="runs on a CUDA"):      # (the draw of a module without a device follows the tensor)
        aug(x)
    with pytest.raises(ValueError, match="channel_axis"):
        jpeg_compress(x, 50, channel_axis=2)
    for wrong in ("422", 1, 4, None, True, 2.0):
        with pytest.raises(ValueError, match="subsampling must be one of"):
            jpeg_compress(x, 50, subsampling=wrong)
    with pytest.raises(ValueError, match="a masked JPEG round trip takes planar"):
        jpeg_compress(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), 50, channel_axis=-1, mask="luminosity")
    with pytest.raises(ValueError, match="luminosity_threshold"):
        jpeg_compress(x, 50, luminosity_threshold=0.0)


def test_sample_rows():
    n = 6000
    aug = JPEGAugment((30, 95), generator=torch.Generator().manual_seed(77))
    rows = aug.sample_rows(n, "cpu")
    assert tuple(rows.shape) == (n,) and rows.dtype == torch.float32 and bool(torch.isfinite(rows).all())
    assert torch.equal(rows, rows.round()) and float(rows.min()) == 30.0 and float(rows.max()) == 95.0      # integers; both ends are drawn
    assert abs(float(rows.mean()) - 62.5) <= 4.0 * ((66.0**2 - 1.0) / 12.0 / n) ** 0.5      # centred: 4 standard errors of a uniform over 66 integers
    # the restated draw: floor(lo + (hi + 1 - lo) * u) capped at hi, u = rand(n) -- a seeded generator reproduces
    again = torch.Generator().manual_seed(77)
    u = torch.rand((n,), generator=again, dtype=torch.float32)
    assert torch.equal(rows, torch.floor(30 + 66 * u).clamp(max=95.0))
    assert torch.equal(JPEGAugment((30, 95), generator=torch.Generator().manual_seed(77)).sample_rows(n, "cpu"), rows)
    # lo == hi: exactly that quality, whatever was drawn
    assert torch.equal(JPEGAugment((42, 42)).sample_rows(7, "cpu"), torch.full((7,), 42.0, dtype=torch.float32))
    assert set(JPEGAugment((99, 100)).sample_rows(400, "cpu").tolist()) == {99.0, 100.0}
    # p < 1: one more draw, rand(n) < p, in that order; a tile that is not chosen gets a NaN quality
    some = JPEGAugment((30, 95), p=0.3, generator=torch.Generator().manual_seed(77))
    rows_p = some.sample_rows(n, "cpu")
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.3
    assert tuple(rows_p.shape) == (n,) and torch.equal(torch.isnan(rows_p), ~chosen)
    assert torch.equal(rows_p[chosen], rows[chosen])
    share = float(chosen.float().mean())
    assert abs(share - 0.3) <= 4.0 * (0.3 * 0.7 / n) ** 0.5, share      # 4 standard errors of a binomial share
    assert bool(torch.isnan(JPEGAugment(p=0.0).sample_rows(9, "cpu")).all()) and bool(torch.isfinite(JPEGAugment(p=1.0).sample_rows(9, "cpu")).all())
