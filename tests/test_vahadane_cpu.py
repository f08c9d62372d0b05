"""Vahadane stain estimation without a GPU: the three entry points are declared, exported by both libraries and bound with matching
arity; every argument error at the C ABI returns its code before anything is enqueued and every Python ValueError is raised before the
backend is touched; the coding step of the float64 restatement satisfies the KKT conditions of the two-variable non-negative lasso; the
iteration descends and reaches a fixed point on real tissue; and the fixed point is scikit-learn's DictionaryLearning's."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from stainx_amd import Macenko, StainEstimate, Vahadane, _native, stain_basis
from tests import _vahadane_numpy as vn

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_vahadane_workspace_bytes": 4, "sx_vahadane_estimate": 18, "sx_stain_max_concentrations": 15}
FAKE, FAKE2, FAKE3, FAKE4, WS = 1 << 40, 1 << 41, 3 << 40, 5 << 40, 7 << 40      # (never dereferenced: every call below fails its checks first)
BAD, DTYPE, WORKSPACE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE, _native.SX_ERR_WORKSPACE


def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search(r"(?:int|size_t) " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert _native.require().sx_version() == 1 and _native.require_diag().sx_version() == 1
    assert "Vahadane" in stainx_amd.__all__ and stainx_amd.Vahadane is Vahadane and stainx_amd.normalizers.Vahadane is Vahadane
    assert issubclass(Vahadane, Macenko) and Vahadane.engine == "VahadaneHIP"


def test_c_abi_rejects_bad_arguments_before_any_launch():
    u8 = _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):
        need = lib.sx_vahadane_workspace_bytes(u8, 4, 64, 64)
        assert need > 0 and need % 256 == 0
        assert lib.sx_vahadane_workspace_bytes(u8, 0, 64, 64) == 0 and lib.sx_vahadane_workspace_bytes(u8, 4, -1, 64) == 0

        def est(images=FAKE, dtype=u8, n=4, h=64, w=64, mask=None, pooled=0, init=FAKE2, n_init=1, lam=0.1, iterations=30, he=FAKE3, max_c=FAKE4, pixels=None, flags=0, ws=WS,
                nbytes=need):
            return lib.sx_vahadane_estimate(images, dtype, n, h, w, mask, pooled, init, n_init, lam, iterations, he, max_c, pixels, flags, ws, nbytes, None)

        def maxc(images=FAKE, dtype=u8, n=4, h=64, w=64, mask=None, pooled=0, he=FAKE2, n_sources=1, max_c=FAKE4, pixels=None, flags=0, ws=WS, nbytes=need):
            return lib.sx_stain_max_concentrations(images, dtype, n, h, w, mask, pooled, he, n_sources, max_c, pixels, flags, ws, nbytes, None)

        def said(word):
            return word in _native.last_error(lib)

        assert est(images=None) == BAD and said("images")
        assert est(init=None) == BAD and said("init_he")
        assert est(he=None) == BAD and said("he_out")
        assert maxc(images=None) == BAD and said("images")
        assert maxc(he=None) == BAD and said("he")
        assert maxc(max_c=None) == BAD and said("max_c_out")
        for call in (est, maxc):
            assert call(n=0) == BAD and call(n=-2) == BAD and call(h=0) == BAD and call(h=-1) == BAD and call(w=0) == BAD and call(w=-7) == BAD
            assert call(n=1 << 40) == BAD and said("overflow")
            assert call(h=1 << 40, w=1 << 40) == BAD and said("overflow")
            assert call(n=1 << 30, h=1 << 15, w=1 << 15, nbytes=1 << 62) == BAD and said("overflow")
            assert call(dtype=17) == DTYPE and call(dtype=-1) == DTYPE and said("dtype")
            for flags in (_native.MACENKO_CHANNELS_LAST, _native.MACENKO_NORMALIZE_0_1, _native.MACENKO_SAMPLED, _native.MACENKO_OUT_BF16, 1 << 20,
                          _native.MACENKO_CLASSIC | _native.MACENKO_CHANNELS_LAST):
                assert call(flags=flags) == BAD and said("flags"), flags
            assert call(ws=None) == WORKSPACE and call(nbytes=need - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE and said("workspace")
            assert call(ws=WS + 64) == WORKSPACE and said("aligned")
        for iterations in (0, -1, 1001, 1 << 20):
            assert est(iterations=iterations) == BAD and said("iterations"), iterations
        for lam in (-0.1, -1e-30, float("inf"), float("-inf"), float("nan")):
            assert est(lam=lam) == BAD and said("lambda"), lam
        for n_init in (0, 2, 3, 5, -1):
            assert est(n_init=n_init) == BAD and said("n_init"), n_init
            assert maxc(n_sources=n_init) == BAD and said("n_sources"), n_init
        assert est(n_init=4, pooled=1) == BAD and said("n_init")      # (pooled: one row)
        assert maxc(n_sources=4, pooled=1) == BAD and said("n_sources")


def test_python_validation_before_the_backend_is_touched():
    images = torch.zeros(2, 3, 8, 8)
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="regularizer"):
            Vahadane(device="cpu", regularizer=bad)
    for bad in (0, -1, 1001, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="iterations"):
            Vahadane(device="cpu", iterations=bad)
    for bad in ("hed", "macenko", torch.zeros(3, 3), torch.zeros(2, 3), torch.zeros(0, 3, 2), torch.zeros(2, 2, 3, 2), np.zeros((3, 2)), None, 1.0):
        with pytest.raises(ValueError, match="init"):
            Vahadane(device="cpu", init=bad)
    with pytest.raises(ValueError, match="mask"):
        Vahadane(device="cpu", mask="otsu")
    with pytest.raises(ValueError, match="luminosity_threshold"):
        Vahadane(device="cpu", luminosity_threshold=1.5)
    with pytest.raises(TypeError):
        Vahadane(device="cpu", precision="fast")      # (there is no precision argument)
    norm = Vahadane(device="cpu")
    assert norm.mask == "luminosity" and norm.regularizer == 0.1 and norm.iterations == 30 and norm.init == "he" and norm._engine is None
    assert Vahadane(device="cpu", mask=None).mask is None
    Vahadane(device="cpu", init=StainEstimate(torch.zeros(1, 3, 2), torch.zeros(1, 2), None))
    for value in (torch.zeros(3, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, 3), np.zeros((2, 8, 8))):
        for call in (norm.estimate, norm.fit, lambda x: norm.max_concentrations(x, torch.zeros(3, 2)), norm.separate):
            with pytest.raises(ValueError, match="expects NCHW"):
                call(value)
    with pytest.raises(ValueError, match="channel_axis"):
        norm.estimate(torch.zeros(2, 8, 8, 3), channel_axis=-1)
    with pytest.raises(ValueError, match="channel_axis"):
        norm.max_concentrations(torch.zeros(2, 8, 8, 3), torch.zeros(3, 2), channel_axis=-1)
    with pytest.raises(ValueError, match="fit"):
        norm.transform(images)
    with pytest.raises(ValueError, match="fit"):
        norm.separate(images, own_basis=False)
    with pytest.raises(ValueError, match="stains, concentrations"):
        norm.separate(images, stains=False, concentrations=False)
    for bad in (torch.zeros(3, 3), torch.zeros(3, 3, 2), torch.zeros(2, 2), None):
        with pytest.raises(ValueError, match="stain_matrices"):
            norm.max_concentrations(images, bad)
    with pytest.raises(ValueError, match="stain_matrices"):
        norm.max_concentrations(images, torch.zeros(2, 3, 2), pooled=True)
    per_tile = Vahadane(device="cpu", init=torch.ones(3, 3, 2))
    with pytest.raises(ValueError, match="init holds 3"):
        per_tile.estimate(images)
    with pytest.raises(ValueError, match="init holds 3"):
        per_tile.estimate(torch.zeros(3, 3, 8, 8), pooled=True)
    for bad_mask in (torch.zeros(2, 8, 8), torch.zeros(2, 8, 9, dtype=torch.uint8), "otsu", 1):
        with pytest.raises(ValueError, match="mask"):
            norm.estimate(images, mask=bad_mask)
    assert norm._engine is None      # (nothing above reached the backend)


def kkt_violation(w: np.ndarray, v: np.ndarray, h: np.ndarray, lam: float) -> float:
    """The largest violation of the KKT conditions of min 0.5 |v - W h|^2 + lam 1.h over h >= 0: with the gradient
    q = W^T (W h - v) + lam, q_i = 0 where h_i > 0 and q_i >= 0 where h_i = 0."""
    q = w.T @ (w @ h - v) + lam
    worst = 0.0
    for i in range(2):
        worst = max(worst, abs(q[i]) if h[i] > 0.0 else max(0.0, -q[i]))
    return max(worst, float(max(0.0, -h.min())))


def test_coding_step_satisfies_the_kkt_conditions():
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(4000):
        w = np.abs(rng.normal(size=(3, 2)))
        if trial % 4 == 0:      # atoms nearly parallel: g close to 1 (d stays above 1e-6)
            w[:, 1] = w[:, 0] + rng.uniform(2e-3, 2e-2) * np.abs(rng.normal(size=3))
        w = vn.normalise_columns(w)
        if 1.0 - float(w[:, 0] @ w[:, 1]) ** 2 <= 1e-5:      # (parallel atoms, d <= 1e-6, skip the two-atom candidate by definition: not the exact lasso)
            continue
        v = rng.normal(size=(3, 1)) * rng.choice([0.05, 0.5, 3.0]) + (0.0 if trial % 3 == 0 else rng.uniform(0.0, 1.5))      # negative entries included
        lam = float(rng.choice([0.0, 0.01, 0.1, 0.7]))
        h = vn.code(w, v, lam)
        scale = 1.0 / (1.0 - float(w[:, 0] @ w[:, 1]) ** 2)      # the candidate's conditioning
        worst = max(worst, kkt_violation(w, v[:, 0], h[:, 0], lam) / scale)
    assert worst < 1e-12, worst


@pytest.fixture(scope="module")
def crops():
    images = vn.real_images()
    return [vn.optical_density(images[i, :, 300:396, 400:480]).reshape(3, -1) for i in range(images.shape[0])]


def test_descent_and_fixed_point_on_real_crops(crops):
    for v in crops:
        w = vn.normalise_columns(vn.HE_INIT)
        last = None
        for _ in range(200):
            h = vn.code(w, v, 0.1)
            now = vn.objective(w, h, v, 0.1)
            assert last is None or now <= last * (1.0 + 1e-13), (last, now)
            w = vn.dictionary_step(w, v, h)
            last = vn.objective(w, h, v, 0.1)
            assert last <= now * (1.0 + 1e-13), (now, last)
        step = np.abs(vn.dictionary_step(w, v, vn.code(w, v, 0.1)) - w).max()
        assert step < 1e-9, step
        assert np.all(w >= 0.0) and np.allclose((w * w).sum(axis=0), 1.0, atol=1e-12)


@pytest.mark.parametrize("index", range(6))
def test_fixed_point_is_scikit_learns(index):
    """0.05 degrees per stain vector.  The margin covers scikit-learn's stopping rule, a relative change of its objective below ``tol``:
    0.0004 .. 0.024 degrees observed at tol=1e-9 (48 .. 248 of its iterations), at most 0.0074 at 1e-10, 0.0007 at 1e-12.  Its coding step
    is a Python loop over the 4000 samples, which is what this test's time goes into."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    rng = np.random.default_rng(5 + index)
    od = vn.optical_density(vn.real_images()[index, :, 256:768, 256:768]).reshape(3, -1)
    v = od[:, rng.choice(od.shape[1], 4000, replace=False)]
    mine = vn.rounds(v, vn.HE_INIT, 0.1, 2000)
    w0 = vn.normalise_columns(vn.HE_INIT)
    # scikit-learn: X (n, 3) ~ code (n, 2) @ dictionary (2, 3), 0.5 |X - C D|^2 + alpha |C|_1, atoms of norm <= 1
    model = decomposition.DictionaryLearning(n_components=2, alpha=0.1, fit_algorithm="cd", transform_algorithm="lasso_cd", positive_dict=True, positive_code=True,
                                             dict_init=w0.T.copy(), code_init=vn.code(w0, v, 0.1).T.copy(), max_iter=2000, tol=1e-9)
    theirs = model.fit(v.T).components_.T
    assert model.n_iter_ < 2000      # (it stopped by its own rule)
    for j in range(2):
        angle = vn.angle_degrees(mine[:, j], theirs[:, j])
        print(f"image {index} stain {j}: {angle:.5f} degrees after {model.n_iter_} scikit-learn iterations")
        assert angle < 0.05, (index, j, angle)
