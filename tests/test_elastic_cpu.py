"""The elastic warp without a GPU: the two entry points are declared and exported, their argument errors at the C ABI return before
anything is enqueued, the float64 restatement of the rule (tests/_elastic_numpy.py) is held to ``scipy.interpolate.BSpline`` and to the
affine restatement (a constant grid is a shift, a grid linear in the control index is an affine row), the rule in float32 stays inside the
band the GPU test uses, and ``elastic_grid_shape`` / ``elastic_grids`` / ``simard_parameters`` / ``ElasticAugment`` do what they say."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import AffineAugment, ElasticAugment, _native, elastic_grid_shape, elastic_grids, elastic_warp, elastic_warp_mask, simard_parameters
from tests import _elastic_numpy as en
from tests import _warp_numpy as wn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_elastic_warp": 18, "sx_elastic_warp_mask": 15}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
TOL = 1e-9      # two float64 evaluations of the same sums
CELLS = (4, 7, 16, 64, 4096)
CASES = (((1, 1), None), ((1, 7), None), ((2, 2), None), ((5, 3), None), ((33, 31), None), ((64, 64), None), ((65, 130), None), ((144, 128), None), ((33, 31), (17, 40)),
         ((33, 31), (40, 40)), ((64, 64), (24, 24)))
CASE_IDS = [f"{s[0]}x{s[1]}" + (f"_to_{o[0]}x{o[1]}" if o else "") for s, o in CASES]


def rows_for(shape, out) -> list:
    """The identity, 30 and 45 degrees with scale and shear, a zoom, a translation several tile widths outside."""
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
    for define in ("SX_ELASTIC_MIN_CELL 4", "SX_ELASTIC_MAX_CELL 4096"):
        assert "#define " + define in header, define
    assert (_native.ELASTIC_MIN_CELL, _native.ELASTIC_MAX_CELL) == (stainx_amd.elastic.MIN_CELL, stainx_amd.elastic.MAX_CELL) == (4, 4096)
    for name in ("ElasticAugment", "elastic_warp", "elastic_warp_mask", "elastic_grids", "elastic_grid_shape", "simard_parameters"):
        assert name in stainx_amd.__all__ and getattr(stainx_amd, name) is getattr(stainx_amd.elastic, name)
    assert isinstance(ElasticAugment(), torch.nn.Module) and callable(elastic_warp)
    source = (ROOT / "stainx_amd" / "csrc" / "elastic.hpp").read_text()
    for function in ("elastic_cell", "elastic_weights", "elastic_sum", "elastic_block_span"):      # written once, for the kernels and the host check
        assert re.search(r"__host__ __device__ inline \w+ " + function + r"\(", source), function
    macenko = (ROOT / "stainx_amd" / "csrc" / "macenko.hip").read_text()
    assert macenko.index('#include "warp.hpp"') < macenko.index('#include "elastic.hpp"')


@pytest.mark.parametrize("which", ["product", "diag"])
def test_calls_reject_bad_arguments_before_any_launch(which):
    lib = _native.require() if which == "product" else _native.require_diag()
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    cl, classic, unit, bf16, f16 = (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_CLASSIC, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_OUT_BF16, _native.MACENKO_OUT_F16)

    def call(images=FAKE, out=FAKE, dtype=f32, n=3, h=8, w=8, oh=8, ow=8, rows=FAKE, n_rows=3, grids=FAKE, n_grids=3, cell=16, interpolation=1, border=0, fill=0.0, flags=0):
        return lib.sx_elastic_warp(images, out, dtype, n, h, w, oh, ow, rows, n_rows, grids, n_grids, cell, interpolation, border, fill, flags, None)

    def mask(images=FAKE, out=FAKE, n=3, h=8, w=8, oh=8, ow=8, rows=FAKE, n_rows=3, grids=FAKE, n_grids=3, cell=16, border=1, fill=0):
        return lib.sx_elastic_warp_mask(images, out, n, h, w, oh, ow, rows, n_rows, grids, n_grids, cell, border, fill, None)

    for fn in (call, mask):
        for name in ("images", "out", "rows", "grids"):
            assert fn(**{name: None}) == BAD and "null" in _native.last_error(lib), name
        assert fn(grids=None) == BAD and "grids pointer is null" in _native.last_error(lib)
        for size in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": -1}, {"oh": 0}, {"ow": -3}):
            assert fn(**size) == BAD and "positive" in _native.last_error(lib), size
        assert fn(n=1 << 20, h=1 << 10, w=1 << 10, n_rows=1, n_grids=1) == BAD and "2^32" in _native.last_error(lib)
        assert fn(n=1 << 20, oh=1 << 10, ow=1 << 10, n_rows=1, n_grids=1) == BAD and "2^32" in _native.last_error(lib)
        for rows in (0, 2, 4, -1):
            assert fn(n_rows=rows) == BAD and "n_rows" in _native.last_error(lib), rows
            assert fn(n_grids=rows) == BAD and "n_grids" in _native.last_error(lib), rows
        for cell in (-1, 0, 3, 4097, 1 << 20):
            assert fn(cell=cell) == BAD and "cell" in _native.last_error(lib), cell
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
    assert call(dtype=17) == DTYPE and call(dtype=17, n_rows=1, n_grids=1, flags=classic | unit | cl) == DTYPE and call(dtype=-1) == DTYPE
    # the order: affine_warp_common's, then the grids, n_grids and the cell, then the fill, the flags, the dtype
    assert call(n=0, n_rows=2) == BAD and "positive" in _native.last_error(lib)
    assert call(n_rows=2, interpolation=9) == BAD and "n_rows" in _native.last_error(lib)
    assert call(interpolation=9, grids=None) == BAD and "interpolation" in _native.last_error(lib)
    assert call(border=9, n_grids=2) == BAD and "border" in _native.last_error(lib)
    assert call(grids=None, n_grids=2) == BAD and "null" in _native.last_error(lib)
    assert call(n_grids=2, cell=1) == BAD and "n_grids" in _native.last_error(lib)
    assert call(cell=1, fill=float("nan")) == BAD and "cell" in _native.last_error(lib)
    assert call(fill=float("nan"), flags=1 << 20) == BAD and "fill" in _native.last_error(lib)
    assert call(flags=1 << 20, dtype=17) == BAD
    assert mask(cell=1, fill=256) == BAD and "cell" in _native.last_error(lib)


# ------------------------------------------------------------------ the restatement against scipy's B-spline and against the affine rule
@pytest.mark.parametrize("cell", CELLS + (5, 33))
def test_spline_of_the_restatement_is_scipys_bspline(cell):
    from scipy.interpolate import BSpline

    for out in ((1, 1), (5, 3), (33, 31), (65, 130), (40, 40)):
        gh, gw = en.grid_shape(out, cell)
        assert (gh, gw) == elastic_grid_shape(out, cell)
        grid = en.test_grids(out, cell, (2.0,))[0]
        knots_x, knots_y = (np.arange(gw + 4) - 3.0) * cell, (np.arange(gh + 4) - 3.0) * cell      # basis j is centred at (j - 1) cell
        xs, ys = np.arange(out[1], dtype=np.float64), np.arange(out[0], dtype=np.float64)
        got = en.displacement(grid, out, cell)
        for plane in range(2):
            across = BSpline(knots_x, grid[plane].astype(np.float64).T, 3)(xs)      # (OW, GH)
            want = BSpline(knots_y, across.T, 3)(ys)      # (OH, OW)
            err = float(np.abs(got[plane] - want).max())
            print(f"spline against scipy, cell {cell}, output {out}, plane {plane}: max |diff| {err:.3e} pixels")
            assert err <= TOL, (cell, out, plane, err)
    t = np.linspace(0.0, 1.0, 101)[:-1]
    w = en.weights(t)
    assert np.abs(w.sum(axis=0) - 1.0).max() <= 1e-15 and (w >= 0.0).all()      # a partition of unity, no negative weight
    squares = (en.weights(np.linspace(0.0, 1.0, 100001)) ** 2).sum(axis=0)
    assert abs(squares.mean() - 151.0 / 315.0) <= 1e-6 and abs(squares.min() - 0.4603) <= 1e-3 and abs(squares.max() - 0.5) <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_constant_grid_is_a_shift_and_linear_grid_is_an_affine_row(case):
    """A cubic B-spline reproduces constants and linear functions: with control j at (j - 1) cell, P[i][j] = al (j - 1) cell + be (i - 1) cell
    + ga gives the displacement al x + be y + ga.  Dyadic numbers: the sums of the rows stay exact in float32."""
    shape, out = case
    out_size = out or shape
    rng = np.random.default_rng(41 + shape[0] * 131 + shape[1])
    planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
    row = np.array((0.75, -0.5, 3.0625, 0.5, 0.75, -2.1875), dtype=np.float32)
    for cell in CELLS:
        gh, gw = en.grid_shape(out_size, cell)
        j, i = np.meshgrid((np.arange(gw) - 1.0) * cell, (np.arange(gh) - 1.0) * cell)
        constant = np.stack([np.full((gh, gw), 1.25), np.full((gh, gw), -2.5)]).astype(np.float32)
        linear = np.stack([0.125 * j - 0.0625 * i + 0.5, 0.03125 * j + 0.25 * i - 1.75]).astype(np.float32)
        shifted = row + np.array((0, 0, 1.25, 0, 0, -2.5), dtype=np.float32)
        sheared = row + np.array((0.125, -0.0625, 0.5, 0.03125, 0.25, -1.75), dtype=np.float32)
        for border, fill in (("mirror", 0.0), ("constant", 37.0)):
            for grid, same_as in ((constant, shifted), (linear, sheared), (np.zeros_like(linear), row)):
                got = en.warp64(planes, row, grid, cell, out, border=border, fill=fill)
                want = wn.warp64(planes, same_as, out, border=border, fill=fill)
                sx, sy = en.coords(row, grid, out_size, cell)
                ax, ay = wn.coords(same_as, *out_size)
                assert max(np.abs(sx - ax).max(), np.abs(sy - ay).max()) <= 1e-9 * max(1.0, np.abs(ax).max(), np.abs(ay).max())
                # (a coordinate that is an integer on one side and a hair below it on the other takes other taps with fractions near 1: the same value)
                err = float(np.abs(got - want).max())
                assert err <= TOL, (case, cell, border, err)
    nan_row = (float("nan"),) * 6      # a tile that is left: the grid is not read
    garbage = np.full((2, *en.grid_shape(out_size, 7)), np.float32(np.nan))
    assert np.array_equal(en.warp64(planes, nan_row, garbage, 7, out), wn.warp64(planes, nan_row, out))


def test_displacements_that_are_not_finite_or_huge_give_fill():
    planes = np.arange(1.0, 3 * 33 * 31 + 1).reshape(3, 33, 31)
    for value in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        grid = np.full((2, *en.grid_shape((33, 31), 7)), np.float32(value))
        for interpolation in ("bilinear", "nearest"):
            for border in ("mirror", "constant"):
                assert (en.warp64(planes, wn.IDENTITY, grid, 7, interpolation=interpolation, border=border, fill=99.0) == 99.0).all(), (value, interpolation, border)


# ------------------------------------------------------------------ the rule in float32 inside the derived band
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_float32_rule_stays_inside_the_derived_band(case):
    """The rule in numpy float32 -- t, the weights, the two sums, the add, the fractions and the three steps as the kernel takes them --
    against float64: every coordinate within ``coordinate_band``, every value within ``value_band`` (printed).  And nearest: the pixels
    within the coordinate band of a half-integer, which the GPU test leaves out, are at most 1 % of a tile at magnitudes <= 3."""
    shape, out = case
    out_size = out or shape
    rng = np.random.default_rng(shape[0])
    planes = rng.integers(0, 256, size=(3, *shape)).astype(np.float64)
    p32 = planes.astype(np.float32)
    for cell in CELLS:
        grids = en.test_grids(out_size, cell)
        for k, row in enumerate(rows_for(shape, out)):
            grid = grids[k % 3]
            sx, sy = en.coords32(row, grid, out_size, cell)
            wx, wy = en.coords(row, grid, out_size, cell)
            e_x, e_y = en.coordinate_band(row, grid, out_size)
            err_x, err_y = float(np.abs(sx.astype(np.float64) - wx).max()), float(np.abs(sy.astype(np.float64) - wy).max())
            print(f"float32 coordinates, {shape} -> {out_size}, cell {cell}, row {k}: {err_x:.3e} of {e_x:.3e}, {err_y:.3e} of {e_y:.3e} pixels")
            assert sx.dtype == np.float32 and err_x <= e_x and err_y <= e_y, (case, cell, k)
            x0, y0 = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0, sy - y0
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            for border in ("mirror", "constant"):
                v = [wn._tap(p32, yi + dy, xi + dx, border, np.float32(7.0)).astype(np.float32) for dy in (0, 1) for dx in (0, 1)]
                top, bot = wn._fma32(fx, v[1] - v[0], v[0]), wn._fma32(fx, v[3] - v[2], v[2])
                got = wn._fma32(fy, bot - top, top)
                want = en.warp64(planes, row, grid, cell, out, border=border, fill=7.0)
                band = en.value_band(row, grid, out_size, True) - 0.5      # (levels, before the rounding to one)
                err = float(np.abs(got.astype(np.float64) - want).max())
                assert err <= band, (case, cell, k, border, err, band)
            unsure = (np.abs(wx - np.floor(wx) - 0.5) <= e_x) | (np.abs(wy - np.floor(wy) - 0.5) <= e_y)
            assert unsure.sum() <= 0.01 * unsure.size or unsure.size < 100, (case, cell, k, int(unsure.sum()))


# ------------------------------------------------------------------ the Python layer
def test_elastic_grid_shape_and_the_draw_of_elastic_grids():
    assert elastic_grid_shape((512, 512), 16) == (35, 35) and elastic_grid_shape((1, 1), 4) == (4, 4) and elastic_grid_shape((224, 320), 4096) == (4, 4)
    assert elastic_grid_shape((33, 31), 7) == (8, 8) and elastic_grid_shape((65, 130), 64) == (5, 6) and elastic_grid_shape((4097, 4096), 4096) == (5, 4)
    for size, cell, what in (((0, 4), 16, "size must be"), (None, 16, "size must be"), ((8, 8), 3, "cell must be an int in 4..4096"), ((8, 8), 4097, "cell must be"), ((8, 8), 16.0, "cell must be"),
                             ((8, 8), True, "cell must be")):
        with pytest.raises(ValueError, match=what):
            elastic_grid_shape(size, cell)
    # ONE draw: randn((n, 2, GH, GW)) with the generator, times the magnitude
    n, size, cell = 5, (65, 130), 16
    got = elastic_grids(n, size, cell, 2.5, generator=torch.Generator().manual_seed(11))
    z = torch.randn((n, 2, *elastic_grid_shape(size, cell)), generator=torch.Generator().manual_seed(11), dtype=torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 2, 8, 12) and torch.equal(got, z * 2.5)
    per_tile = torch.tensor([0.0, 1.0, 2.0, 0.5, 3.0])
    assert torch.equal(elastic_grids(n, size, cell, per_tile, generator=torch.Generator().manual_seed(11)), z * per_tile.view(n, 1, 1, 1))
    assert not bool(elastic_grids(n, size, cell, 0.0).any())
    for magnitude, what in ((-1.0, "magnitude must be finite and >= 0"), (float("nan"), "magnitude must be"), ("x", "magnitude must be a number"), (torch.zeros(4), r"shape \(\) or \(N,\) = \(5,\)")):
        with pytest.raises(ValueError, match=what):
            elastic_grids(n, size, cell, magnitude)
    with pytest.raises(ValueError, match="n must be a positive int"):
        elastic_grids(0, size, cell, 1.0)


def test_simard_parameters_are_the_two_derivations():
    cell, magnitude = simard_parameters(100.0, 10.0)
    assert cell == 17 and magnitude == pytest.approx(100.0 / (math.sqrt(3.0) * 2.0 * math.sqrt(math.pi) * 10.0) * 315.0 / 151.0, rel=1e-12)
    assert simard_parameters(34.0, 1.0)[0] == 4 and simard_parameters(1.0, 4.0)[0] == 7 and simard_parameters(1.0, 1e6)[0] == 4096      # (kept within 4..4096)
    assert simard_parameters(0.0, 4.0)[1] == 0.0
    for args, what in (((-1.0, 4.0), "alpha must be finite and >= 0"), ((1.0, 0.0), "sigma must be finite and positive"), ((1.0, float("inf")), "sigma must be"), (("a", 1.0), "alpha must be a number")):
        with pytest.raises(ValueError, match=what):
            simard_parameters(*args)


def test_simard_field_and_spline_field_have_the_same_standard_deviation():
    """alpha = 100, sigma = 10 on 1024 x 1024: ``alpha * gaussian_filter(U(-1, 1), sigma)`` against the spline field of
    ``simard_parameters``' grid.  The margin is statistical: a field smoothed over sigma has about H W / (4 pi sigma^2) = 834 independent
    values, its sample standard deviation a relative standard error of 1 / sqrt(2 * 834) = 2.4 %; the difference of two such fields, at four
    standard errors: 4 * sqrt(2) * 2.4 % = 14 %, and 1 % for the truncated Gaussian and the rounded cell: 15 %.  Each also lies within
    10 % (four standard errors and that 1 %) of the derived 1.629."""
    from scipy import ndimage

    alpha, sigma, side = 100.0, 10.0, 1024
    rng = np.random.default_rng(2003)
    simard = alpha * ndimage.gaussian_filter(rng.uniform(-1.0, 1.0, size=(side, side)), sigma)
    cell, magnitude = simard_parameters(alpha, sigma)
    grid = elastic_grids(1, (side, side), cell, magnitude, generator=torch.Generator().manual_seed(2003))[0].numpy()
    dx, dy = en.displacement(grid, (side, side), cell)
    derived = alpha / (math.sqrt(3.0) * 2.0 * math.sqrt(math.pi) * sigma)
    got_simard, got_spline = float(simard.std()), float(np.sqrt(0.5 * (dx.var() + dy.var())))
    print(f"standard deviation at alpha {alpha}, sigma {sigma}: derived {derived:.3f}, Simard field {got_simard:.3f}, spline field (cell {cell}, magnitude {magnitude:.3f}) {got_spline:.3f} pixels")
    assert abs(got_simard - got_spline) <= 0.15 * derived, (got_simard, got_spline)
    assert abs(got_simard - derived) <= 0.10 * derived and abs(got_spline - derived) <= 0.10 * derived, (got_simard, got_spline, derived)


def test_constructor_validation_names_the_argument():
    for kwargs, what in (({"magnitude": 2.0}, "magnitude must be a"), ({"magnitude": (2.0, 1.0)}, "lo <= hi"), ({"magnitude": (-1.0, 1.0)}, "magnitude lo must be finite and >= 0"),
                         ({"magnitude": (0.0, float("inf"))}, "magnitude hi"), ({"cell": 3}, "cell must be an int in 4..4096"), ({"cell": 8.0}, "cell must be"), ({"affine": "yes"}, "affine must be None or an AffineAugment"),
                         ({"affine": AffineAugment(size=(8, 8)), "size": (9, 9)}, "size comes from affine"), ({"p": 1.5}, "p must"), ({"size": (0, 4)}, "size must be"),
                         ({"interpolation": "bicubic"}, "interpolation must be one of"), ({"border": "wrap"}, "border must be one of"), ({"fill": float("inf")}, "fill must be finite"),
                         ({"device": "cpu"}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            ElasticAugment(**kwargs)
    aug = ElasticAugment((0.5, 2.5), 32, affine=AffineAugment(size=(224, 224)), p=0.5, interpolation="nearest", border="constant", fill=255)
    assert aug.size == (224, 224) and aug.cell == 32 and aug.magnitude == (0.5, 2.5)
    text = repr(aug)
    for part in ("magnitude=(0.5, 2.5)", "cell=32", "affine=AffineAugment(...)", "p=0.5", "size=(224, 224)", "interpolation='nearest'", "border='constant'", "fill=255.0", "normalize_to_0_1=True"):
        assert part in text, part
    assert "cell=16" in repr(ElasticAugment()) and "affine=None" in repr(ElasticAugment())


def test_argument_errors_come_before_gpu_work():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    grids, rows = torch.zeros(4, 2, 4, 4), torch.zeros(4, 6)
    aug = ElasticAugment(cell=16)
    for fn in (lambda img, g, **k: elastic_warp(img, g, cell=16, **k), lambda img, g, **k: aug(img, g, **k)):
        with pytest.raises(ValueError, match="expects a tensor"):
            fn(x.numpy(), grids)
        with pytest.raises(ValueError, match="expects CHW / NCHW"):
            fn(torch.zeros(4, 8, 8, 3, dtype=torch.uint8), grids)
        for wrong in (torch.zeros(4, 2, 4, 5), torch.zeros(2, 2, 4, 4), torch.zeros(4, 3, 4, 4), torch.zeros(2, 4), [0.0]):
            with pytest.raises(ValueError, match=r"grids must be a tensor of shape \(2, GH, GW\), \(1, 2, GH, GW\) or \(N, 2, GH, GW\) = \(4, 2, 4, 4\)"):
                fn(x, wrong)
        with pytest.raises(ValueError, match=r"rows must be a tensor of shape \(6,\), \(1, 6\) or \(N, 6\) = \(4, 6\)"):
            fn(x, grids, rows=torch.zeros(3, 6))
        for fine in (grids, grids[:1], grids[0]):      # everything above came first: only now would the GPU be touched
            with pytest.raises(ValueError, match="runs on a CUDA"):
                fn(x, fine)
            with pytest.raises(ValueError, match="runs on a CUDA"):
                fn(x, fine, rows=rows)
        with pytest.raises(ValueError, match="runs on a CUDA"):      # a CHW tile: N = 1
            fn(x[0], grids[0])
    with pytest.raises(ValueError, match="rows= goes with grids="):
        aug(x, None, rows)
    with pytest.raises(ValueError, match="runs on a CUDA"):      # (the draw of a module without a device follows the tensor)
        aug(x)
    for kwargs, what in (({"cell": 3}, "cell must be"), ({"cell": 8, "size": (0, 8)}, "size must be"), ({"cell": 16, "size": (40, 8)}, "grids must be"), ({"cell": 16, "interpolation": "cubic"}, "interpolation must be one of"),
                         ({"cell": 16, "border": "edge"}, "border must be one of"), ({"cell": 16, "fill": float("nan")}, "fill must be finite"), ({"cell": 16, "channel_axis": 2}, "channel_axis"),
                         ({"cell": 16, "out_dtype": torch.float64}, "out_dtype is supported for uint8 input")):
        with pytest.raises(ValueError, match=what):
            elastic_warp(x, grids, **kwargs)
    with pytest.raises(TypeError):      # cell is required
        elastic_warp(x, grids)
    with pytest.raises(ValueError, match="runs on a CUDA"):
        elastic_warp(torch.zeros(4, 8, 8, 3), torch.zeros(2, 5, 5), cell=4, channel_axis=-1, size=(5, 6), interpolation="nearest", border="constant", fill=3.0)
    for wrong, what in ((torch.ones(4, 8, 8), "mask dtype"), (torch.ones(4, 8, 9, dtype=torch.uint8), "mask shape"), ("luminosity", "expects a tensor")):
        with pytest.raises(ValueError, match=what):
            aug(x, grids, mask=wrong)
    m = torch.ones(4, 8, 8, dtype=torch.uint8)
    for args, kwargs, what in (((m.numpy(), grids), {}, "expects a tensor"), ((m.float(), grids), {}, "mask dtype"), ((m[0], grids), {}, "mask shape"), ((m, grids[:3]), {}, "grids must be a tensor"),
                               ((m, grids), {"rows": rows[:3]}, "rows must be a tensor"), ((m, grids), {"size": (3, -1)}, "size must be"), ((m, grids), {"border": "reflect"}, "border must be one of"),
                               ((m, grids), {"fill": 256}, "fill must be an int in 0..255"), ((m, grids), {}, "runs on a CUDA"), ((m.bool().unsqueeze(1), grids[0]), {"border": "mirror", "fill": 255, "rows": rows[0]}, "runs on a CUDA")):
        with pytest.raises(ValueError, match=what):
            elastic_warp_mask(*args, cell=16, **kwargs)


def test_sample_keeps_its_order_and_its_where_logic():
    n, in_size, size = 400, (320, 320), (224, 224)
    anchor = torch.tensor(wn.anchor_row(*in_size, *size))
    # without affine: rand(n) for the magnitudes, randn for the grids, rand(n) < p; rows: the anchor row where chosen, NaN otherwise
    aug = ElasticAugment((0.5, 2.5), 16, p=0.4, size=size, generator=torch.Generator().manual_seed(9))
    rows, grids = aug.sample(n, in_size, "cpu")
    again = torch.Generator().manual_seed(9)
    u = torch.rand((n,), generator=again, dtype=torch.float32)
    z = torch.randn((n, 2, *elastic_grid_shape(size, 16)), generator=again, dtype=torch.float32)
    chosen = torch.rand((n,), generator=again, dtype=torch.float32) < 0.4
    assert 0.25 * n < int(chosen.sum()) < 0.55 * n
    want = z * (0.5 + 2.0 * u.double()).float().view(n, 1, 1, 1)
    assert grids.dtype == torch.float32 and torch.equal(grids[chosen], want[chosen]) and not bool(grids[~chosen].any())      # a tile that is not chosen: a ZERO grid
    assert torch.equal(rows[chosen], anchor.expand(int(chosen.sum()), 6)) and bool(torch.isnan(rows[~chosen]).all())
    everything = ElasticAugment((1.0, 1.0), 16, size=size, generator=torch.Generator().manual_seed(9)).sample(n, in_size, "cpu")      # p = 1: no third draw, every tile chosen
    assert torch.equal(everything[0], anchor.expand(n, 6)) and torch.equal(everything[1], z)
    # with affine: its sample_rows comes first, with ITS generator; a chosen tile whose affine row is NaN gets the anchor row, a tile with neither keeps its NaN row
    make_affine = lambda: AffineAugment((-30.0, 30.0), scale=(0.8, 1.25), p=0.5, size=size, generator=torch.Generator().manual_seed(3))  # noqa: E731
    both = ElasticAugment((0.5, 2.5), 16, affine=make_affine(), p=0.4, generator=torch.Generator().manual_seed(9))
    rows, grids = both.sample(n, in_size, "cpu")
    given = make_affine().sample_rows(n, in_size, "cpu")
    left = torch.isnan(given).any(dim=1)
    assert bool((left & chosen).any()) and bool((left & ~chosen).any()) and bool((~left & chosen).any()) and bool((~left & ~chosen).any())
    assert torch.equal(grids[chosen], want[chosen]) and not bool(grids[~chosen].any())
    assert torch.equal(rows[~left], given[~left])      # affine's rows as they are, chosen or not
    assert torch.equal(rows[left & chosen], anchor.expand(int((left & chosen).sum()), 6))
    assert bool(torch.isnan(rows[left & ~chosen]).all())      # neither change: the copy path (or the centre crop)
    assert both.size == size and rows.dtype == torch.float32 and tuple(grids.shape) == (n, 2, 17, 17)
