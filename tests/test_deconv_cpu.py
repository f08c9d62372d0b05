"""Three-stain colour deconvolution without a GPU: the built-in bases and the complement, the identities of the float64 restatement
(tests/_deconv_numpy.py), the input condition of the uint8 GPU cases, the C ABI's declarations and argument errors, and the Python
surface's argument errors (raised before any GPU work)."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stainx_amd
from oracle import stain_oracle as so
from stainx_amd import ColorDeconvolution, HEDAugment, StainEstimate, _native, complement_basis, stain_basis
from tests import _deconv_numpy as dn
from tests import _masked_numpy as mn
from tests.conftest import load_golden

ROOT = Path(__file__).resolve().parents[1]
CALLS = {"sx_deconv_apply": 14, "sx_deconv_apply_masked": 15, "sx_deconv_separate": 11, "sx_deconv_combine": 10}
FAKE = 1 << 40      # (256-byte aligned, never dereferenced: every call below fails its checks first)
BAD, DTYPE = _native.SX_ERR_BAD_ARG, _native.SX_ERR_DTYPE
TOL_255 = 2.55e-2      # tests/test_macenko_gpu.py
LOOSE_SHARE = 0.12     # tests/test_macenko_mask_gpu.py: the cap of the uint8 rule on levels that lie within TOL_255 of an integer
NAMES = ("hed", "he", "hdab")
TABLE = {"hed": [(0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78)], "he": [(0.644211, 0.716556, 0.266844), (0.092789, 0.954111, 0.283111)],
         "hdab": [(0.650, 0.704, 0.286), (0.268, 0.570, 0.776)]}


def macenko_golden_he() -> np.ndarray:
    """Every per-tile HE_source of the committed Macenko goldens: (K, 3, 2) float32."""
    rows = []
    for name in ("g1_macenko_64x64.npz", "g1_macenko_128x128.npz", "g1_macenko_321x199.npz"):
        g = load_golden(name)
        rows += [g["f32_he"], g["u8_he"]]
    rows.append(load_golden("g2_macenko_config2.npz")["he"])
    return np.concatenate(rows).astype(np.float32)


# ------------------------------------------------------------------------------------------------ bases
def test_named_bases_have_unit_columns_and_are_well_conditioned():
    for name in NAMES:
        b = stain_basis(name)
        assert b.shape == (3, 3) and b.dtype == torch.float32 and b.device.type == "cpu"
        m = b.double().numpy()
        np.testing.assert_allclose(np.linalg.norm(m, axis=0), 1.0, atol=1e-6)
        for s, vec in enumerate(TABLE[name]):      # the tabulated vectors, normalised, as columns
            v = np.asarray(vec) / np.linalg.norm(vec)
            np.testing.assert_allclose(m[:, s], v, atol=1e-6, err_msg=f"{name} column {s}")
        if len(TABLE[name]) == 2:      # the third: the complement
            np.testing.assert_allclose(m[:, 2], dn.complement(m[:, :2])[:, 2], atol=1e-6)
        det, cond = np.linalg.det(m), np.linalg.cond(m)
        print(f"{name}: det {det:.4f}, condition number {cond:.3f}")
        assert abs(det) > 0.2 and cond <= 4.0, (name, det, cond)
    with pytest.raises(ValueError, match="unknown stain basis"):
        stain_basis("vahadane")


def test_given_bases_are_checked_on_the_host():
    good = torch.tensor([[2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [1.0, 0.0, 4.0]])
    b = stain_basis(good)
    np.testing.assert_allclose(np.linalg.norm(b.numpy(), axis=0), 1.0, atol=1e-6)
    assert stain_basis(good.numpy().tolist()).shape == (3, 3)
    assert stain_basis(torch.stack([good, good])).shape == (2, 3, 3)
    for bad, what in ((torch.rand(3, 2), "shape"), (torch.rand(2, 3, 2), "shape"), (torch.full((3, 3), float("nan")), "finite"),
                      (torch.tensor([[1.0, 2.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]), "invertible"), (torch.zeros(3, 3), "invertible"), (object(), "name")):
        with pytest.raises(ValueError, match=what):
            stain_basis(bad)


def test_complement_basis():
    he = torch.from_numpy(macenko_golden_he())
    full = complement_basis(he)
    assert full.shape == (he.shape[0], 3, 3) and full.dtype == torch.float32
    assert torch.equal(full[..., :2], he)      # the two stain vectors as they are
    m = full.double().numpy()
    third = m[..., 2]
    np.testing.assert_allclose(np.linalg.norm(third, axis=-1), 1.0, atol=1e-6)
    assert np.abs(np.einsum("kc,kcs->ks", third, m[..., :2])).max() <= 1e-6      # orthogonal to both
    assert (np.linalg.det(m) > 0).all()      # right-handed
    worst = 0.0
    for k in range(he.shape[0]):      # inverse(complement(HE)) rows 0-1: the oracle's pseudo-inverse (its least-squares solution of HE C = I)
        pinv = so.concentrations(he[k].numpy(), np.eye(3, dtype=np.float32))
        worst = max(worst, float(np.abs(np.linalg.inv(m[k])[:2] - pinv).max()))
    print(f"|inverse(complement(HE))[:2] - pinv(HE)| over {he.shape[0]} golden estimates: {worst:.2e} (bound 1e-6)")
    assert worst <= 1e-6
    assert complement_basis(he[0]).shape == (3, 3)
    est = StainEstimate(he[:4], torch.rand(4, 2), None)
    assert torch.equal(est.complement(), full[:4]) and StainEstimate(he[0], torch.rand(2), None).complement().shape == (1, 3, 3)
    with pytest.raises(ValueError, match="3, 2"):
        complement_basis(torch.rand(4, 2, 3))


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_identities():
    x8 = mn.real_crops(64)[:3].numpy()
    xf = (x8.astype(np.float32) / np.float32(255.0))
    e = np.eye(3)
    for name in NAMES:
        basis = stain_basis(name).numpy()
        for x in (x8, xf):
            unit = so.to_unit_float(x).astype(np.float64)
            want = unit * 255.0 + 1.0      # 240 exp(-OD) of the untouched optical density
            got = dn.apply(x, basis, dtype=np.float64)
            np.testing.assert_allclose(got, want, rtol=1e-9)
            conc = dn.concentrations(x, basis)
            np.testing.assert_allclose(dn.combine(conc, basis, dtype=np.float64), want, rtol=1e-9)
            images = dn.stain_images(x, basis, dtype=np.float64)
            for s in range(3):
                alone = dn.apply(x, basis, alpha=e[s][None], beta=np.zeros((1, 3)), dtype=np.float64)
                np.testing.assert_allclose(images[s], alone, rtol=1e-9)
            # the three images' product over 240^2 is the tile again (exp(-a - b - c))
            np.testing.assert_allclose(images[0] * images[1] * images[2] / 240.0**2, want, rtol=1e-9)
    # per-tile bases and one row for the batch
    per_tile = np.stack([stain_basis(n).numpy() for n in NAMES])
    a = dn.apply(x8, per_tile, alpha=[dn.ALPHA], beta=[dn.BETA])
    for i, name in enumerate(NAMES):
        np.testing.assert_array_equal(a[i], dn.apply(x8[i : i + 1], stain_basis(name).numpy(), alpha=[dn.ALPHA], beta=[dn.BETA])[0])
    # a mask copies, a NaN row copies the tile, and what lies under the mask does not matter
    mask = np.zeros((3, 64, 64), dtype=bool)
    mask[:, 8:40, 16:] = True
    nan_rows = per_tile.copy()
    nan_rows[1, 2, 0] = np.nan
    m = dn.apply(xf, nan_rows, alpha=[dn.ALPHA], beta=[dn.BETA], mask=mask)
    keep = np.broadcast_to(mask[:, None], xf.shape)
    np.testing.assert_array_equal(m[~keep], dn.input_levels(xf)[~keep])
    np.testing.assert_array_equal(m[1], dn.input_levels(xf)[1])
    np.testing.assert_array_equal(m[0][keep[0]], dn.apply(xf[:1], per_tile[:1], alpha=[dn.ALPHA], beta=[dn.BETA])[0][keep[0]])
    y = xf.copy()
    y[~keep] = np.nan
    np.testing.assert_array_equal(dn.apply(y, nan_rows, alpha=[dn.ALPHA], beta=[dn.BETA], mask=mask)[keep], m[keep])


def test_uint8_cases_keep_the_near_integer_share_under_the_cap():
    """The uint8 rule of the GPU tests compares exactly where the restated level is farther than TOL_255 from an integer and within one
    level elsewhere; it holds only while the second kind stays a small share (LOOSE_SHARE).  A condition on the INPUT: the 256 x 256
    crops of the six real images with alpha = (1.15, 0.9, 1.05), beta = (0.02, -0.03, 0.01), asserted per tile for the three bases.
    (alpha = (0.85, 1.2, 0.95), beta = (-0.04, 0.03, 0.02) with "hdab" is NOT usable: one tile reaches 0.142.  The identity is not
    usable on uint8 either: every level is then an integer.)"""
    x = mn.real_crops(256).numpy()
    worst = 0.0
    for name in NAMES:
        levels = dn.apply(x, stain_basis(name).numpy(), alpha=[dn.ALPHA], beta=[dn.BETA])
        shares = [dn.near_integer_share(levels[i], TOL_255) for i in range(x.shape[0])]
        print(f"{name}: near-integer share of the restated levels per tile {[round(s, 3) for s in shares]} (cap {LOOSE_SHARE})")
        worst = max(worst, max(shares))
        assert max(shares) <= LOOSE_SHARE, (name, shares)
    print(f"worst share {worst:.3f}")
    # the smaller uint8 apply cases, and the stain images of every uint8 separate case (one stain alone has a share of its own)
    for what, tiles, bases in dn.uint8_apply_cases(x)[1:]:
        for name in bases:
            share = dn.near_integer_share(dn.apply(np.ascontiguousarray(tiles), stain_basis(name).numpy(), alpha=[dn.ALPHA], beta=[dn.BETA]), TOL_255)
            print(f"apply {what} {name}: near-integer share {share:.3f} (cap {LOOSE_SHARE})")
            assert share <= LOOSE_SHARE, (what, name, share)
    for what, tiles, bases in dn.uint8_separate_cases(x):
        for name in bases:
            images = dn.stain_images(np.ascontiguousarray(tiles), stain_basis(name).numpy())
            shares = [dn.near_integer_share(images[s], TOL_255) for s in range(3)]
            print(f"stain images {what} {name}: near-integer shares {[round(v, 3) for v in shares]} (cap {LOOSE_SHARE})")
            assert max(shares) <= LOOSE_SHARE, (what, name, shares)
    # the anchor of the GPU tests against sx_macenko_apply: the tiles' own estimates, complemented, the third factor zeroed
    od = so.optical_density(so.to_unit_float(x))
    full = dn.complement(np.stack([so.macenko_tile_params(od[i])["he"] for i in range(x.shape[0])])).astype(np.float32)
    a, b = np.array([dn.ALPHA] * x.shape[0]), np.array([dn.BETA] * x.shape[0])
    a[:, 2] = b[:, 2] = 0.0
    share = dn.near_integer_share(dn.apply(x, full, alpha=a, beta=b), TOL_255)
    print(f"anchor (complemented estimates, third factor 0): near-integer share {share:.3f} (cap {LOOSE_SHARE})")
    assert share <= LOOSE_SHARE


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exported_by_both_libraries_and_declared():
    header = (ROOT / "include" / "stainx_hip.h").read_text()
    for name, params in CALLS.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == params, name
        for path in (_native.LIB_PATH, _native.DIAG_LIB_PATH):
            assert hasattr(ctypes.CDLL(str(path)), name), (name, path)
        decl = re.search("int " + name + r"\((.*?)\);", header, flags=re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == params, name
    assert "#define SX_ABI_VERSION 1" in header      # (additions only)
    assert "SINGULAR basis is NOT detected" in header


def test_calls_reject_bad_arguments_before_any_launch():
    f32, u8 = _native.DTYPE_CODES[torch.float32], _native.DTYPE_CODES[torch.uint8]
    for lib in (_native.require(), _native.require_diag()):

        def apply(images=FAKE, out=FAKE, dtype=f32, n=4, basis=FAKE, n_bases=4, target=FAKE, n_targets=1, alpha=FAKE, beta=FAKE, flags=0):
            return lib.sx_deconv_apply(images, out, dtype, n, 64, 64, basis, n_bases, target, n_targets, alpha, beta, flags, None)

        def apply_masked(images=FAKE, out=FAKE, dtype=f32, n=4, basis=FAKE, n_bases=4, target=FAKE, n_targets=1, alpha=FAKE, beta=FAKE, mask=FAKE, flags=0):
            return lib.sx_deconv_apply_masked(images, out, dtype, n, 64, 64, basis, n_bases, target, n_targets, alpha, beta, mask, flags, None)

        def separate(images=FAKE, stains=FAKE, conc=FAKE, dtype=f32, n=4, basis=FAKE, n_bases=4, flags=0):
            return lib.sx_deconv_separate(images, stains, conc, dtype, n, 64, 64, basis, n_bases, flags, None)

        def combine(images=FAKE, out=FAKE, dtype=f32, n=4, basis=FAKE, n_bases=4, flags=0):
            return lib.sx_deconv_combine(images, out, dtype, n, 64, 64, basis, n_bases, flags, None)

        for call in (apply, apply_masked, separate, combine):
            assert call(images=None) == BAD and "null" in _native.last_error(lib), call.__name__
            assert call(flags=_native.MACENKO_CLASSIC, basis=None) == BAD and "basis" in _native.last_error(lib)      # (CLASSIC is accepted: the next check answers)
            assert call(n=0) == BAD and call(dtype=17) == DTYPE, call.__name__
            for n_bases in (0, 2, 3, 5, -1):
                assert call(n_bases=n_bases) == BAD and "n_bases" in _native.last_error(lib), (call.__name__, n_bases)
            for flags in (_native.MACENKO_SAMPLED, 1 << 20, _native.MACENKO_NO_TIE_SHORTCUT):
                assert call(flags=flags) == BAD and "flags" in _native.last_error(lib), (call.__name__, flags)
        for call in (apply, apply_masked, separate):
            assert call(flags=_native.MACENKO_OUT_BF16) == BAD and call(dtype=u8, flags=_native.MACENKO_OUT_BF16 | _native.MACENKO_OUT_F16) == BAD, call.__name__
        for call in (apply, apply_masked):
            assert call(out=None) == BAD
            assert call(alpha=None) == BAD and "alpha and beta" in _native.last_error(lib)
            assert call(beta=None) == BAD and "alpha and beta" in _native.last_error(lib)
            for n_targets in (0, 2, 3, 5, -1):
                assert call(n_targets=n_targets) == BAD and "n_targets" in _native.last_error(lib), (call.__name__, n_targets)
        assert apply_masked(mask=None) == BAD and "mask" in _native.last_error(lib)
        assert apply_masked(flags=_native.MACENKO_CHANNELS_LAST) == BAD and "planar" in _native.last_error(lib)
        assert separate(stains=None, conc=None) == BAD and "both null" in _native.last_error(lib)
        assert combine(out=None) == BAD
        assert combine(flags=_native.MACENKO_OUT_BF16) == BAD and combine(dtype=u8, flags=_native.MACENKO_NORMALIZE_0_1) == BAD


# ------------------------------------------------------------------------------------------------ the Python surface
BAD_MASKS = [(torch.ones(4, 8, 10, dtype=torch.float32), "dtype"), (torch.ones(4, 10, 8, dtype=torch.uint8), "shape"), (torch.ones(3, 8, 10, dtype=torch.uint8), "shape"),
             (torch.ones(4, 8, 10, dtype=torch.uint8), "device"), (np.ones((4, 8, 10), dtype=np.uint8), "tensor"), ("otsu", "mask")]


def test_public_surface():
    assert {"ColorDeconvolution", "HEDAugment", "stain_basis", "complement_basis", "DeconvSeparation"} <= set(stainx_amd.__all__)
    from stainx_amd.backends.torch_hip_backend import DeconvHIP, TorchHIPBackendBase

    assert issubclass(DeconvHIP, TorchHIPBackendBase)
    assert isinstance(HEDAugment(), torch.nn.Module)


def test_python_arguments_are_refused_before_any_gpu_work():
    x = torch.zeros(4, 3, 8, 10, dtype=torch.uint8)
    for kwargs, what in (({"basis": "vahadane"}, "unknown stain basis"), ({"basis": torch.zeros(3, 3)}, "invertible"), ({"target": torch.rand(3, 2)}, "shape"),
                         ({"channel_axis": 0}, "channel_axis"), ({"device": "cpu"}, "CUDA"), ({"mask": "otsu"}, "mask"), ({"luminosity_threshold": 1.5}, "luminosity_threshold"),
                         ({"mask": "luminosity", "channel_axis": -1}, "planar")):
        with pytest.raises(ValueError, match=what):
            ColorDeconvolution(**kwargs)
    cd = ColorDeconvolution("hdab", device="cuda")
    with pytest.raises(ValueError, match="C=3"):
        cd.apply(torch.zeros(4, 8, 10, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="C=3"):
        cd.separate(torch.zeros(8, 10))
    with pytest.raises(ValueError, match="tensor"):
        cd.apply(np.zeros((4, 3, 8, 10), dtype=np.uint8))
    with pytest.raises(ValueError, match="stains=True"):
        cd.separate(x, stains=False)
    with pytest.raises(ValueError, match="both or neither"):
        cd.apply(x, alpha=torch.ones(4, 3))
    for a, b in ((torch.ones(4, 2), torch.zeros(4, 3)), (torch.ones(4, 3), torch.zeros(3, 3)), (torch.ones(12), torch.zeros(12))):
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            cd.apply(x, alpha=a, beta=b)
    for mask, what in BAD_MASKS:
        with pytest.raises(ValueError, match=what):
            cd.apply(x, mask=mask)
    with pytest.raises(ValueError, match="planar"):
        ColorDeconvolution(device="cuda", channel_axis=-1).apply(torch.zeros(4, 8, 10, 3, dtype=torch.uint8), mask="luminosity")
    with pytest.raises(ValueError, match="bases for a batch"):
        ColorDeconvolution(torch.stack([stain_basis("hed")] * 3), device="cuda").apply(x)
    with pytest.raises(ValueError, match="float32"):
        cd.combine(torch.zeros(4, 3, 8, 10, dtype=torch.float64))
    with pytest.raises(ValueError, match="out_dtype"):
        cd.combine(torch.zeros(4, 3, 8, 10), out_dtype=torch.int32)
    with pytest.raises(ValueError, match="float out_dtype"):
        ColorDeconvolution(device="cuda", normalize_to_0_1=True).combine(torch.zeros(4, 3, 8, 10))
    with pytest.raises(ValueError, match="CUDA"):      # a CPU tensor and no device: refused, never computed on the CPU
        ColorDeconvolution().apply(x)
    # HEDAugment
    for kwargs, what in (({"sigma1": 1.0}, "sigma1"), ({"sigma1": (0.1, 0.1)}, "sigma1"), ({"sigma2": -0.1}, "sigma2"), ({"sigma2": "x"}, "sigma2"), ({"basis": "vahadane"}, "unknown"),
                         ({"device": "cpu"}, "CUDA"), ({"mask": "otsu"}, "mask")):
        with pytest.raises(ValueError, match=what):
            HEDAugment(**kwargs)
    aug = HEDAugment(device="cuda")
    with pytest.raises(ValueError, match="C=3"):
        aug(torch.zeros(4, 8, 10, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        aug(x, alpha=torch.ones(4, 2), beta=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="device"):
        aug(x, alpha=torch.ones(4, 3), beta=torch.zeros(4, 3), mask=torch.ones(4, 8, 10, dtype=torch.uint8))


def test_sample_factors_are_seeded_and_per_stain():
    aug = HEDAugment((0.1, 0.0, 0.3), (0.0, 0.02, 0.05), generator=torch.Generator().manual_seed(7))
    a1, b1 = aug.sample_factors(64)
    aug.generator.manual_seed(7)
    a2, b2 = aug.sample_factors(64)
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and a1.shape == (64, 3) and b1.dtype == torch.float32
    assert (a1[:, 1] == 1.0).all() and (b1[:, 0] == 0.0).all()      # sigma = 0: exactly 1 and 0
    assert ((a1[:, 0] - 1).abs() <= 0.1 + 1e-6).all() and ((a1[:, 2] - 1).abs() <= 0.3 + 1e-6).all() and ((a1[:, 2] - 1).abs() > 0.1).any()
    assert (b1[:, 1].abs() <= 0.02 + 1e-7).all() and (b1[:, 2].abs() <= 0.05 + 1e-7).all()
    a0, b0 = HEDAugment(0.0, 0.0).sample_factors(5)
    assert (a0 == 1.0).all() and (b0 == 0.0).all()
