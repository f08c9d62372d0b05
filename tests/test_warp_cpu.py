"""The affine warp without a GPU: the two entry points are declared and exported, their argument errors at the C ABI return before
anything is enqueued, the float64 restatement of the rule (tests/_warp_numpy.py) is held to ``scipy.ndimage.affine_transform`` (order 1
and 0, ``mirror`` and ``grid-constant``), the small rules (fold, anchor row, coordinate limit) are held at their boundaries, the rule in
float32 stays inside the band the GPU test derives, ``affine_rows`` keeps its three conventions and its exact quarter turns, and
``affine_warp`` / ``affine_warp_mask`` / ``AffineAugment`` validate and draw what they say."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import AffineAugment, _native, affine_rows, affine_warp, affine_warp_mask
from tests import _warp_numpy as wn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_affine_warp": 15, "sx_affine_warp_mask": 12}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
SCIPY_TOL = 1e-9      # two float64 evaluations of the same sums
CASES = (((1, 1), None), ((1, 7), None), ((2, 2), None), ((5, 3), None), ((33, 31), None), ((65, 130), None), ((33, 31), (17, 40)), ((33, 31), (40, 40)), ((64, 64), (24, 24)))
CASE_IDS = [f"{s[0]}x{s[1]}" + (f"_to_{o[0]}x{o[1]}" if o else "") for s, o in CASES]
DYADIC_ROWS = ((0.75, -0.5, 3.0625, 0.5, 0.75, -2.1875), (1.0, 0.0, 2.0, 0.0, 1.0, -3.0), (1.0, 0.0, 0.25, 0.0, 1.0, -1.75), (0.0, -1.0, 30.0, 1.0, 0.0, 0.0), (0.5, 0.0, 0.5, 0.0, 0.5, 0.5))


def rows_for(shape, out) -> list:
    """Identity, 30 and 45 degrees with scale and shear, a zoom, a translation several tile widths outside."""
    h, w = shape
    return [wn.IDENTITY, *wn.rows64(3, shape, out, angle=(30.0, 45.0, 0.0), scale=(1.2, 0.7, 1.9), shear=(10.0, -5.0, 0.0), translate=((1.5, -2.25, 0.3), (0.0, 4.0, -0.7))),
            (1.0, 0.0, 3.25 * w + 0.4, 0.0, 1.0, -4.5 * h - 0.3)]


def test_declared_exported_and_public():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    for define in ("SX_WARP_NEAREST 0", "SX_WARP_BILINEAR 1", "SX_WARP_MIRROR 0", "SX_WARP_CONSTANT 1", "SX_WARP_MAX_COORD 4194304.0f"):
        assert "#define " + define in header, define
    assert _native.WARP_INTERPOLATIONS == {"nearest": 0, "bilinear": 1} and _native.WARP_BORDERS == {"mirror": 0, "constant": 1}
    assert stainx_amd.warp.MAX_COORD == wn.MAX_COORD == _native.WARP_MAX_COORD == 2.0**22
    for name in ("AffineAugment", "affine_warp", "affine_warp_mask", "affine_rows"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.warp, name)
    assert isinstance(AffineAugment(), torch.nn.Module) and callable(affine_warp)
    source = (ROOT / "stainx_amd" / "csrc" / "warp.hpp").read_text()
    assert "#define SX_WARP_MAX_COORD 4194304.0f" in source and "__host__ __device__ inline WarpTaps warp_taps" in source


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, oh=8, ow=8, rows=FAKE, n_rows=3, interpolation=1, border=0, fill=0.0, flags=0):
        return lib.sx_affine_warp(images, out, dtype, n, h, w, oh, ow, rows, n_rows, interpolation, border, fill, flags, None)

    def mask(images=FAKE, out=FAKE, n=3, h=8, w=8, oh=8, ow=8, rows=FAKE, n_rows=3, border=1, fill=0):
        return lib.sx_affine_warp_mask(images, out, n, h, w, oh, ow, rows, n_rows, border, fill, None)

    for fn in (call, mask):
        for name in ("images", "out", "rows"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        for size in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": -1}, {"oh": 0}, {"ow": -3}):
            assert fn(**size) == BAD and "positive" in _native.last_error(lib), size
        assert fn(n=1 << 20, h=1 << 10, w=1 << 10, n_rows=1) == BAD and "2^32" in _native.last_error(lib)
        assert fn(n=1 << 20, oh=1 << 10, ow=1 << 10, n_rows=1) == BAD and "2^32" in _native.last_error(lib)
        for rows in (0, 2, 4, -1):
            assert fn(n_rows=rows) == BAD and "n_rows" in _native.last_error(lib), rows
        for border in (-1, 2, 7):
            assert fn(border=border) == BAD and "border" in _native.last_error(lib), border
    for interpolation in (-1, 2, 3):
        assert call(interpolation=interpolation) == BAD and "interpolation" in _native.last_error(lib), interpolation
    for fill in (float("nan"), float("inf"), float("-inf")):
        assert call(fill=fill) == BAD and "fill must be finite" in _native.last_error(lib), fill
    for fill in (-1, 256, 1000):
        assert mask(fill=fill) == BAD and "0..255" in _native.last_error(lib), fill
    for flags in (_native.MACENKO_SAMPLED, 1 << 20, _native.MACENKO_TWO_PASS, bf16, f16):      # (the output flags: uint8 input only)
        assert call(flags=flags) == BAD, flags
    assert call(dtype=u8, flags=bf16 | f16) == BAD      # (one of the two)
    assert call(dtype=17) == DTYPE and call(dtype=17, n_rows=1, flags=classic | unit | cl) == DTYPE and call(dtype=-1) == DTYPE
    # the order: the sizes before the rows, the rows before the interpolation, the fill before the flags, everything before the dtype
    assert call(n=0, n_rows=2) == BAD and "positive" in _native.last_error(lib)
    assert call(n_rows=2, interpolation=9) == BAD and "n_rows" in _native.last_error(lib)
    assert call(interpolation=9, fill=float("nan")) == BAD and "interpolation" in _native.last_error(lib)
    assert call(fill=float("nan"), flags=1 << 20) == BAD and "fill" in _native.last_error(lib)
    assert call(flags=1 << 20, dtype=17) == BAD


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_restatement_agrees_with_scipy(case):
    from scipy import ndimage

    shape, out = case
    rng = np.random.default_rng(23 + shape[0] * 131 + shape[1])
    planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
    out_size = out or shape
    for row in rows_for(shape, out):
        matrix, offset = wn.scipy_arguments(row)
        for border, mode, fill in (("mirror", "mirror", 0.0), ("constant", "grid-constant", 37.0)):
            got = wn.warp64(planes, row, out, border=border, fill=fill)
            want = np.stack([ndimage.affine_transform(p, matrix, offset, output_shape=out_size, order=1, mode=mode, cval=fill) for p in planes])
            err = float(np.abs(got - want).max())
            print(f"restatement against scipy, {shape} -> {out_size}, {border}, row {np.round(np.asarray(row, dtype=np.float64), 3).tolist()}: max |diff| {err:.3e} levels")
            assert got.shape == (3, *out_size) and err <= SCIPY_TOL, (shape, out, border, row, err)
            assert got.min() >= min(planes.min(), fill) - 1e-9 and got.max() <= max(planes.max(), fill) + 1e-9      # every step lies between its operands


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_nearest_restatement_equals_scipy_on_dyadic_rows(case):
    """Rows whose entries are multiples of 1/16: the coordinates are exact in float32 -- equal element for element, the ties of the last
    row (every coordinate of it is k + 0.5, k >= 0) included.  (A NEGATIVE tie under "mirror" is where scipy differs: it reflects the
    coordinate first and rounds then; the rule rounds first.  No row here has one.)"""
    from scipy import ndimage

    shape, out = case
    rng = np.random.default_rng(29 + shape[0] * 131 + shape[1])
    planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
    out_size = out or shape
    for row in DYADIC_ROWS:
        sx, sy = wn.coords(row, *out_size)
        sx32, sy32 = wn.coords32(row, *out_size)
        assert np.array_equal(sx, sx32.astype(np.float64)) and np.array_equal(sy, sy32.astype(np.float64))      # exact in float32
        matrix, offset = wn.scipy_arguments(row)
        for border, mode, fill in (("mirror", "mirror", 0.0), ("constant", "grid-constant", 37.0)):
            got = wn.nearest(planes, row, out, border=border, fill=fill)
            want = np.stack([ndimage.affine_transform(p, matrix, offset, output_shape=out_size, order=0, mode=mode, cval=fill) for p in planes])
            assert np.array_equal(got, want), (shape, out, border, row)
            assert np.array_equal(wn.warp64(planes, row, out, interpolation="nearest", border=border, fill=fill), got)


# ------------------------------------------------------------------ the small rules
def test_fold_is_numpys_reflect_padding():
    assert wn.fold(np.arange(-17, 18), 1).tolist() == [0] * 35
    for n in (2, 3, 7, 31):
        pad = 4 * n + 3
        assert wn.fold(np.arange(-pad, n + pad), n).tolist() == np.pad(np.arange(n), pad, mode="reflect").tolist(), n


def test_anchor_row_divides_by_floor_in_both_directions():
    assert wn.anchor_row(10, 10, 10, 10).tolist() == [1, 0, 0, 0, 1, 0]
    assert wn.anchor_row(10, 9, 7, 4).tolist() == [1, 0, 2, 0, 1, 1]      # (9 - 4) div 2 = 2, (10 - 7) div 2 = 1: the centre crop
    assert wn.anchor_row(7, 4, 10, 9).tolist() == [1, 0, -3, 0, 1, -2]      # (4 - 9) div 2 = -3, (7 - 10) div 2 = -2: floor, not truncation
    assert wn.anchor_row(8, 8, 9, 7).tolist() == [1, 0, 0, 0, 1, -1]
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(6):
            row = list(wn.IDENTITY)
            row[k] = bad
            assert np.array_equal(wn.effective_row(row, 7, 4, 10, 9), wn.anchor_row(7, 4, 10, 9)), (bad, k)
    assert np.array_equal(wn.effective_row((3e38, -3e38, 1e-45, 0, 0, 0), 7, 4, 10, 9), np.array((3e38, -3e38, 1e-45, 0, 0, 0), dtype=np.float32))      # finite: kept
    planes = np.arange(3 * 10 * 9, dtype=np.float64).reshape(3, 10, 9)
    nan_row = (float("nan"),) * 6
    assert np.array_equal(wn.warp64(planes, nan_row), planes)      # the copy
    assert np.array_equal(wn.warp64(planes, nan_row, (7, 4)), planes[:, 1:8, 2:6])      # the centre crop
    padded = wn.warp64(planes, nan_row, (13, 12), border="constant", fill=-1.0)      # the centre pad: (9 - 12) div 2 = -2, (10 - 13) div 2 = -2
    assert np.array_equal(padded[:, 2:12, 2:11], planes) and (padded[:, :2] == -1).all() and (padded[:, :, :2] == -1).all() and (padded[:, 12:] == -1).all() and (padded[:, :, 11:] == -1).all()


def test_coordinate_limit_at_its_boundary_floats():
    limit = np.float32(wn.MAX_COORD)
    above, below = np.nextafter(limit, np.float32(np.inf)), np.nextafter(limit, np.float32(0))
    s = np.array([limit, -limit, below, -below, above, -above, np.inf, -np.inf, np.nan, 0.0, 1e30, -1e30], dtype=np.float32)
    assert wn.coord_ok(s).tolist() == [True, True, True, True, False, False, False, False, False, True, False, False]
    planes = np.arange(1.0, 13.0).reshape(1, 3, 4)
    for border in ("mirror", "constant"):
        for interpolation in ("bilinear", "nearest"):
            kw = {"interpolation": interpolation, "border": border, "fill": 99.0}
            assert (wn.warp64(planes, (1e30, 0, 0, 0, 1, 0), **kw)[..., 1:] == 99.0).all()      # column 0 sits at coordinate 0
            assert (wn.warp64(planes, (1, 0, float(above), 0, 1, 0), **kw) == 99.0).all()
            assert (wn.warp64(planes, (1, 0, 0, 0, 1, -float(above) - 2.0), **kw) == 99.0).all()      # rows 0..2 at -(2^22 + 2.5) .. -(2^22 + 0.5)
            at_limit = wn.warp64(planes, (1, 0, float(limit) - 3, 0, 1, 0), **kw)      # columns 0..3 at 2^22 - 3 .. 2^22: inside the limit
            assert (at_limit == 99.0).all() if border == "constant" else np.isin(at_limit, planes).all()


def test_float32_rule_stays_inside_the_derived_band():
    """The rule in numpy float32 -- coordinates, fractions and the three steps as the kernel takes them -- against float64, held to the
    band tests/test_warp_gpu.py derives from the row and the shape: 255 * 2^-23 * (Sx + Sy) + 1e-3 levels (printed)."""
    for shape, out in (((33, 31), None), ((33, 31), (40, 40)), ((65, 130), None), ((144, 128), None)):
        rng = np.random.default_rng(shape[0])
        planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
        oh, ow = out or shape
        for row in rows_for(shape, out):
            for border in ("mirror", "constant"):
                sx, sy = wn.coords32(row, oh, ow)
                x0, y0 = np.floor(sx), np.floor(sy)
                fx, fy = sx - x0, sy - y0
                assert fx.dtype == np.float32
                xi, yi = x0.astype(np.int64), y0.astype(np.int64)
                p32 = planes.astype(np.float32)
                v = [wn._tap(p32, yi + dy, xi + dx, border, np.float32(7.0)).astype(np.float32) for dy in (0, 1) for dx in (0, 1)]
                top, bot = wn._fma32(fx, v[1] - v[0], v[0]), wn._fma32(fx, v[3] - v[2], v[2])
                got = wn._fma32(fy, bot - top, top)
                assert got.dtype == np.float32
                want = wn.warp64(planes, row, out, border=border, fill=7.0)
                s_x, s_y = wn.coordinate_slack(row, oh, ow)
                band = 255.0 * 2.0**-23 * (s_x + s_y) + 1e-3
                err = float(np.abs(got.astype(np.float64) - want).max())
                print(f"float32 rule against float64, {shape} -> {(oh, ow)}, {border}: max |diff| {err:.3e} levels (band {band:.3e})")
                assert err <= band, (shape, out, border, row, err, band)


# ------------------------------------------------------------------ affine_rows
def test_quarter_turns_and_flips_are_rows_of_exact_integers():
    for side in (8, 33):
        for turn in range(-4, 9):
            for flip in (False, True):
                row = affine_rows(1, (side, side), angle=90.0 * turn, flip=flip)[0].double().numpy()
                assert row.dtype == np.float64 and np.array_equal(row, np.round(row)), (side, turn, flip, row)
                assert sorted(np.abs(row[[0, 1, 3, 4]]).tolist()) == [0, 0, 1, 1]
    x = np.arange(3 * 33 * 33, dtype=np.float64).reshape(3, 33, 33)
    for turn in range(4):
        row = affine_rows(1, (33, 33), angle=90.0 * turn)[0].numpy()
        assert np.array_equal(wn.nearest(x, row), np.rot90(x, turn, axes=(-2, -1))), turn      # anticlockwise, as np.rot90 / torch.rot90
        assert np.array_equal(wn.warp64(x, row), np.rot90(x, turn, axes=(-2, -1))), turn      # (bilinear: fx = fy = 0 everywhere)
        flipped = affine_rows(1, (33, 33), angle=90.0 * turn, flip=True)[0].numpy()
        assert np.array_equal(wn.nearest(x, flipped), np.rot90(x[..., ::-1], turn, axes=(-2, -1))), turn      # the flip comes BEFORE the turn
    assert np.array_equal(wn.nearest(x, affine_rows(1, (33, 33), angle=450.0)[0].numpy()), np.rot90(x, 1, axes=(-2, -1)))
    assert torch.equal(affine_rows(1, (8, 8))[0], torch.tensor(wn.IDENTITY))


def test_affine_rows_is_the_restated_formula_within_one_float32_ulp():
    n = 64
    gen = torch.Generator().manual_seed(3)
    angle, scale = torch.rand(n, generator=gen, dtype=torch.float64) * 720 - 360, torch.rand(n, generator=gen, dtype=torch.float64) * 1.5 + 0.5
    shear, tx, ty = torch.rand(n, generator=gen, dtype=torch.float64) * 60 - 30, torch.rand(n, generator=gen, dtype=torch.float64) * 40 - 20, torch.rand(n, generator=gen, dtype=torch.float64) * 40 - 20
    flip = torch.rand(n, generator=gen) < 0.5
    angle[:4] = torch.tensor([0.0, 90.0, -180.0, 270.0], dtype=torch.float64)
    for in_size, out_size in (((320, 320), (224, 224)), ((33, 31), None), ((64, 96), (17, 40))):
        got = affine_rows(n, in_size, out_size, angle=angle, scale=scale, shear=shear, translate=(tx, ty), flip=flip)
        want = wn.rows64(n, in_size, out_size, angle=angle.numpy(), scale=scale.numpy(), shear=shear.numpy(), translate=(tx.numpy(), ty.numpy()), flip=flip.numpy())
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 6)
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        assert (np.abs(got.numpy().astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    # numbers broadcast; a float32 tensor is taken as float64
    assert torch.equal(affine_rows(3, (9, 9), angle=30.0, scale=2.0), affine_rows(3, (9, 9), angle=torch.full((3,), 30.0), scale=torch.tensor(2.0)))
    assert np.array_equal(affine_rows(2, (9, 7), (5, 4), angle=33.0, shear=5.0, translate=(1.0, -2.0)).numpy(), wn.rows64(2, (9, 7), (5, 4), angle=33.0, shear=5.0, translate=(1.0, -2.0)))


def test_the_three_conventions():
    x = np.zeros((1, 65, 65))
    x[0, 32, 48] = 1.0      # a dot to the RIGHT of the centre
    turned = wn.warp64(x, affine_rows(1, (65, 65), angle=90.0)[0].numpy())
    assert turned[0, 16, 32] == 1.0 and turned.sum() == 1.0      # a positive angle turns the content anticlockwise: the dot is ABOVE the centre
    slightly = wn.warp64(x, affine_rows(1, (65, 65), angle=10.0)[0].numpy())
    assert np.unravel_index(slightly.argmax(), slightly.shape)[1] < 32      # ... and at 10 degrees it has moved up
    bigger = wn.warp64(x, affine_rows(1, (65, 65), scale=2.0)[0].numpy())
    assert bigger[0, 32, 64] == 1.0 and bigger.sum() > 2.0      # scale > 1 magnifies: the dot moves outward, to 32 + 2 * 16, and grows
    moved = wn.warp64(x, affine_rows(1, (65, 65), translate=(3.0, -2.0))[0].numpy())
    assert moved[0, 30, 51] == 1.0      # translate moves the content right and down
    y = np.zeros((1, 65, 65))
    y[0, 20, 48] = 1.0      # right of the centre and above it
    both = wn.warp64(y, affine_rows(1, (65, 65), angle=90.0, flip=True)[0].numpy())
    assert both[0, 48, 20] == 1.0      # mirrored first (-> left, above), then turned anticlockwise (-> below, left): the flip comes before the turn
    with pytest.raises(ValueError, match="scale must be finite and positive"):
        affine_rows(1, (8, 8), scale=0.0)
    with pytest.raises(ValueError, match=r"angle must be a number or a tensor of shape \(\) or \(N,\) = \(3,\)"):
        affine_rows(3, (8, 8), angle=torch.zeros(2))
    with pytest.raises(ValueError, match="in_size"):
        affine_rows(1, (8, 0))


# ------------------------------------------------------------------ the module and the functional forms
def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"rotate": 10.0}, "rotate must be a"), ({"rotate": "half"}, "rotate must be a"), ({"rotate": (10.0, -10.0)}, "lo <= hi"), ({"rotate": (float("nan"), 1.0)}, "rotate lo"),
                         ({"scale": (0.0, 1.0)}, "scale lo must be finite and positive"), ({"scale": (1.0, float("inf"))}, "scale hi"), ({"scale": 1.0}, "scale must be a"),
                         ({"shear": (-90.0, 0.0)}, "shear lo"), ({"shear": ("a", 1.0)}, "shear lo must be a number"), ({"translate": 0.1}, "translate must be"),
                         ({"translate": (-0.1, 0.0)}, "translate fx"), ({"translate": (0.0, float("nan"))}, "translate fy"), ({"p": 1.5}, "p must"), ({"p": float("nan")}, "p must"),
                         ({"size": (0, 4)}, "size must be"), ({"size": 224}, "size must be"), ({"size": (2.0, 4)}, "size must be"), ({"interpolation": "bicubic"}, "interpolation must be one of"),
                         ({"border": "wrap"}, "border must be one of"), ({"fill": float("inf")}, "fill must be finite"), ({"fill": "x"}, "fill must be a number"), ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            AffineAugment(**kwargs)
    aug = AffineAugment("quarter", scale=(0.8, 1.25), shear=(-5, 5), translate=(0.1, 0.2), flip=False, p=0.5, size=(224, 224), interpolation="nearest", border="constant", fill=255)
    assert aug.rotate == "quarter" and aug.scale == (0.8, 1.25) and aug.size == (224, 224) and aug.fill == 255.0
    text = repr(aug)
    for part in ("rotate='quarter'", "scale=(0.8, 1.25)", "shear=(-5.0, 5.0)", "translate=(0.1, 0.2)", "flip=False", "p=0.5", "size=(224, 224)", "interpolation='nearest'",
                 "border='constant'", "fill=255.0", "normalize_to_0_1=True"):
        assert part in text, part
    assert "rotate=(-180.0, 180.0)" in repr(AffineAugment()) and "size=None" in repr(AffineAugment())


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    rows = torch.zeros(4, 6)
    aug = AffineAugment()
    for fn in (lambda *a, **k: affine_warp(*a, **k), lambda img, r, **k: aug(img, r, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), rows)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), rows)
        for wrong in (torch.zeros(5), torch.zeros(4, 5), torch.zeros(2, 6), torch.zeros(6, 4), [0.0] * 6):
            with pytest.raises(ValueError, match=r"rows must be a tensor of shape \(6,\), \(1, 6\) or \(N, 6\) = \(4, 6\)"):
                fn(x, wrong)
        for fine in (rows, rows[:1], rows[0]):      # everything above came first: only now would the GPU be touched
            with pytest.raises(ValueError, match="runs on a CUDA"):
                fn(x, fine)
        with pytest.raises(ValueError, match="runs on a CUDA"):      # a CHW tile: N = 1
            fn(x[0], rows[:1])
    with pytest.raises(ValueError, match="runs on a CUDA"):      # (the draw of a module without a device follows the tensor)
        aug(x)
    for kwargs, what in (({"size": (0, 8)}, "size must be"), ({"size": (8,)}, "size must be"), ({"interpolation": "cubic"}, "interpolation must be one of"), ({"border": "edge"}, "border must be one of"),
                         ({"fill": float("nan")}, "fill must be finite"), ({"fill": None}, "fill must be a number"), ({"channel_axis": 2}, "channel_axis"),
                         ({"out_dtype": torch.float64}, "out_dtype is supported for uint8 input")):
        with pytest.raises(ValueError, match=what):
            affine_warp(x, rows, **kwargs)
    with pytest.raises(ValueError, match="out_dtype is supported for uint8 input"):
        affine_warp(x.float(), rows, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        affine_warp(torch.zeros(4, 8, 8, 3), rows, channel_axis=-1, size=(5, 6), interpolation="nearest", border="constant", fill=3.0)
    # the mask that is warped with the tiles
    for wrong, what in ((torch.ones(4, 8, 8), "mask dtype"), (torch.ones(4, 8, 9, dtype=torch.uint8), "mask shape"), (torch.ones(4, 2, 8, 8, dtype=torch.uint8), "mask shape"), ("luminosity", "expects a tensor")):
        with pytest.raises(ValueError, match=what):
            aug(x, rows, mask=wrong)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        aug(x, rows, mask=torch.ones(4, 1, 8, 8, dtype=torch.bool))
    m = torch.ones(4, 8, 8, dtype=torch.uint8)
    for args, kwargs, what in (((m.numpy(), rows), {}, "expects a tensor"), ((m.float(), rows), {}, "mask dtype"), ((m[0], rows), {}, "mask shape"), ((m, rows[:3]), {}, "rows must be a tensor"),
                               ((m, rows), {"size": (3, -1)}, "size must be"), ((m, rows), {"border": "reflect"}, "border must be one of"), ((m, rows), {"fill": 256}, "fill must be an int in 0..255"),
                               ((m, rows), {"fill": 1.0}, "fill must be an int in 0..255"), ((m, rows), {}, "runs on a CUDA"), ((m.bool().unsqueeze(1), rows[0]), {"border": "mirror", "fill": 255}, "runs on a CUDA")):
        with pytest.raises(ValueError, match=what):
            affine_warp_mask(*args, **kwargs)


def test_sample_rows():
    n, size = 4000, (320, 320)
    aug = AffineAugment((-30.0, 60.0), scale=(0.8, 1.25), shear=(-5.0, 10.0), translate=(0.1, 0.05), size=(224, 224), generator=torch.Generator().manual_seed(77))
    rows = aug.sample_rows(n, size, "cpu")
    assert tuple(rows.shape) == (n, 6) and rows.dtype == torch.float32 and bool(torch.isfinite(rows).all())
    # the restated draw: six rand(n) in the documented order -- a seeded generator reproduces
    again = torch.Generator().manual_seed(77)
    u = [torch.rand((n,), generator=again, dtype=torch.float32).double().numpy() for _ in range(6)]
    want = wn.rows64(n, size, (224, 224), angle=-30.0 + 90.0 * u[0], scale=0.8 + (1.25 - 0.8) * u[1], shear=-5.0 + 15.0 * u[2],
                     translate=((2.0 * u[3] - 1.0) * (0.1 * 224), (2.0 * u[4] - 1.0) * (0.05 * 224)), flip=u[5] < 0.5)
    assert (np.abs(rows.numpy().astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert torch.equal(AffineAugment((-30.0, 60.0), scale=(0.8, 1.25), shear=(-5.0, 10.0), translate=(0.1, 0.05), size=(224, 224), generator=torch.Generator().manual_seed(77)).sample_rows(n, size, "cpu"), rows)
    share = float((u[5] < 0.5).mean())
    assert abs(share - 0.5) <= 4.0 * (0.25 / n) ** 0.5, share      # 4 standard errors of a binomial share
    # "quarter": the four right angles, with flips the eight symmetries -- rows of integers on a square tile, all eight drawn
    basic = AffineAugment("quarter", generator=torch.Generator().manual_seed(5)).sample_rows(400, (64, 64), "cpu")
    assert torch.equal(basic, basic.round()) and len({tuple(r) for r in basic.tolist()}) == 8
    assert len({tuple(r) for r in AffineAugment("quarter", flip=False, generator=torch.Generator().manual_seed(5)).sample_rows(400, (64, 64), "cpu").tolist()}) == 4
    # degenerate ranges: exactly that value, whatever was drawn
    assert torch.equal(AffineAugment((0.0, 0.0), flip=False).sample_rows(7, (9, 9), "cpu"), torch.tensor(wn.IDENTITY).repeat(7, 1))
    # p < 1: one more draw, rand(n) < p, after the six; a tile that is not chosen gets a row of NaNs
    some = AffineAugment((-30.0, 60.0), scale=(0.8, 1.25), shear=(-5.0, 10.0), translate=(0.1, 0.05), size=(224, 224), p=0.3, generator=torch.Generator().manual_seed(77))
    rows_p = some.sample_rows(n, size, "cpu")
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.3
    assert torch.equal(torch.isnan(rows_p).all(dim=1), ~chosen) and torch.equal(torch.isnan(rows_p).any(dim=1), ~chosen)
    assert torch.equal(rows_p[chosen], rows[chosen])
    assert bool(torch.isnan(AffineAugment(p=0.0).sample_rows(9, (8, 8), "cpu")).all()) and bool(torch.isfinite(AffineAugment(p=1.0).sample_rows(9, (8, 8), "cpu")).all())
