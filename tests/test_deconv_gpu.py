"""Three-stain colour deconvolution on the GPU (include/stainx_hip.h: sx_deconv_apply / _apply_masked / _separate / _combine): against the
float64 restatement of the contract (tests/_deconv_numpy.py) within the project's own bounds, the identities bit for bit, the anchor
against sx_macenko_apply, the round trip, masks, the plumbing, and the Python surface.

Shapes: odd sizes (33 x 37: the scalar path, one work item; 67 x 65: the scalar path, two work items, the last partial), 64 x 64 (whole
work items), 96 x 84 (= 8064 pixels: with kStreamThreads = 256 and one pack set per work item that is 15.75 work items of float64 packs
of 2, 7.9 of float32 packs of 4, 3.9 of 16-bit packs of 8 and 1.97 of the separation's uint8 packs of 16), 160 x 112 (= 17920 pixels:
1.09 work items of the uint8 -> uint8 apply, 4 pack sets of 16 per thread) and the 256 x 256 real crops.

Measured on an MI355X (the figures this file prints; DESIGN.md 4n quotes them): float32 / float64 images within 2.7e-4 of the restatement
(stain images 3.1e-4, combine 2.3e-4; bound 2.55e-2), concentrations within 1.4e-6 (bound 3e-5), uint8 on the real crops exact away from
near-integers with 18-32 of 1 179 648 values off by one level and a near-integer share of 0.043-0.050 (cap 0.12), bf16 / f16 tiles within
one unit of their format on fewer than 2e-3 of the values."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import ColorDeconvolution, HEDAugment, Macenko, _native, stain_basis, tissue_mask
from tests import _deconv_numpy as dn
from tests import _masked_numpy as mn
from tests.conftest import TORCH_DTYPES
from tests.test_macenko_mask_gpu import HALF_BOUND, HALF_SHARE, LOOSE_SHARE, TOL_255, background_expected, same_bits, unaligned_copy

pytestmark = pytest.mark.gpu

CONC_TOL = 3e-5      # concentrations: the bound of tests/test_separate_apply_gpu.py
NAMES = ("hed", "he", "hdab")
FLAGS = {"unit": _native.MACENKO_NORMALIZE_0_1, "nhwc": _native.MACENKO_CHANNELS_LAST, torch.bfloat16: _native.MACENKO_OUT_BF16, torch.float16: _native.MACENKO_OUT_F16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import DeconvHIP

    return DeconvHIP(dev)


@pytest.fixture(scope="module")
def lib():
    return _native.require()


@pytest.fixture(scope="module")
def real():
    """The six 256 x 256 real crops (uint8, CPU) and the restated levels of apply with the factors of the uint8 cases, per named basis:
    computed once, never changed."""
    x = mn.real_crops(256)
    levels = {name: dn.apply(x.numpy(), stain_basis(name).numpy(), alpha=[dn.ALPHA], beta=[dn.BETA]) for name in NAMES}
    return x, levels


def factors(n: int, dev) -> tuple[torch.Tensor, torch.Tensor]:
    return torch.tensor([dn.ALPHA] * n, dtype=torch.float32, device=dev), torch.tensor([dn.BETA] * n, dtype=torch.float32, device=dev)


def tiles_of(x8: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """uint8 tiles as ``dt``: the unit value u / 255 rounded to the element type (what a decoder followed by ToDtype(scale=True) gives)."""
    return x8 if dt == torch.uint8 else (x8.float() / 255.0).to(dt)


def oracle_in(x: torch.Tensor) -> np.ndarray:
    return x.numpy() if x.dtype in (torch.uint8, torch.float32, torch.float64) else x.float().numpy()


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def check_levels(got: torch.Tensor, levels: np.ndarray, dt: torch.dtype, what) -> float:
    """A plain (0-255) output against restated un-clamped float32 levels by the rule of its element type (check_output of
    tests/test_macenko_mask_gpu.py, over every pixel).  Returns the figure it printed."""
    got = got.cpu()
    if dt in (torch.float32, torch.float64):
        err = float(np.abs(got.double().numpy() - np.clip(levels, 0, 255).astype(np.float64)).max())
        print(f"{what} {dt}: max |out - restated| {err:.3e} (bound {TOL_255})")
        assert err <= TOL_255, what
        return err
    if dt == torch.uint8:
        want = so.restore_dtype(levels, np.uint8, in_0_255=True)
        near = np.abs(levels - np.rint(levels)) <= np.float32(TOL_255)
        g = got.numpy()
        off = int((g != want).sum())
        print(f"{what} uint8: near-integer share {near.mean():.3f} (cap {LOOSE_SHARE}), pixels off by one level {off} of {g.size}")
        assert near.mean() <= LOOSE_SHARE, what
        assert np.array_equal(g[~near], want[~near]), what
        assert np.abs(g.astype(np.int16) - want.astype(np.int16)).max() <= 1, what
        return float(off)
    want = torch.from_numpy(np.clip(levels, 0, 255)).to(dt)
    diff = (got.double() - want.double()).abs().numpy()
    print(f"{what} {dt}: max diff {diff.max()}, share differing {(diff > 0).mean():.2e} (bounds {HALF_BOUND[dt]}, {HALF_SHARE})")
    assert diff.max() <= HALF_BOUND[dt] and (diff > 0).mean() < HALF_SHARE, what
    return float(diff.max())


def unit_of(plain: torch.Tensor, x_dtype: torch.dtype, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """What SX_MACENKO_NORMALIZE_0_1 makes of a plain output, on the CPU: / 255 in float32 (float64: in float64), cast to the output type."""
    p = plain.cpu()
    if x_dtype == torch.float64:
        return p / 255.0
    target = out_dtype if out_dtype is not None else (torch.float32 if x_dtype == torch.uint8 else x_dtype)
    return (p.float() / 255.0).to(target)


# ---- the raw C ABI on caller-owned buffers (misaligned views, poisoned outputs) ----
def raw_apply(lib, x, out, basis, target=None, alpha=None, beta=None, mask=None, flags=0):
    ch_last = bool(flags & _native.MACENKO_CHANNELS_LAST)
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if ch_last else (x.shape[0], x.shape[2], x.shape[3])
    nb = 1 if basis.dim() == 2 else basis.shape[0]
    nt = 0 if target is None else (1 if target.dim() == 2 else target.shape[0])
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    code, stream = _native.DTYPE_CODES[x.dtype], _native.stream_ptr(x.device)
    if mask is None:
        rc = lib.sx_deconv_apply(x.data_ptr(), out.data_ptr(), code, n, h, w, basis.data_ptr(), nb, p(target), nt, p(alpha), p(beta), flags, stream)
    else:
        rc = lib.sx_deconv_apply_masked(x.data_ptr(), out.data_ptr(), code, n, h, w, basis.data_ptr(), nb, p(target), nt, p(alpha), p(beta), mask.data_ptr(), flags, stream)
    _native.check(rc, "sx_deconv_apply", lib)
    return out


def poisoned(shape, dtype, dev) -> torch.Tensor:
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(0xA5)
    return t


def complement_of(x8: torch.Tensor, dev) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-tile Macenko estimates of uint8 tiles and their (N, 3, 3) complements, on the device."""
    est = Macenko(device=dev).estimate(x8.to(dev))
    return est.stain_matrices, est.complement()


# ------------------------------------------------------------------------------------------------ 1. against the restatement
SHAPES = {"33x37": (3, 33, 37), "67x65": (2, 67, 65), "64x64": (4, 64, 64), "96x84": (3, 96, 84)}


@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_apply_against_the_restatement(dev, be, real, name):
    dt = TORCH_DTYPES[name]
    x8, levels = real
    if dt == torch.uint8:      # (the full uint8 rule: the inputs whose near-integer share tests/test_deconv_cpu.py asserts)
        cases = [(what, tiles.contiguous(), levels if what == "real" else None, bases) for what, tiles, bases in dn.uint8_apply_cases(x8)]
    else:
        cases = [("real", x8, None, NAMES)]
        for shape_name, (n, h, w) in SHAPES.items():
            cases.append((shape_name, x8[:n, :, 11 : 11 + h, 5 : 5 + w].contiguous(), None, NAMES if shape_name == "96x84" else ("hdab",)))
    worst = 0.0
    for what, tiles8, restated, bases in cases:
        x = tiles_of(tiles8, dt)
        n = x.shape[0]
        a, b = factors(n, dev)
        for basis_name in bases:
            basis = stain_basis(basis_name).to(dev)
            lv = restated[basis_name] if restated is not None else dn.apply(oracle_in(x), basis.cpu().numpy(), alpha=[dn.ALPHA], beta=[dn.BETA])
            plain = be.apply(x.to(dev), basis, alpha=a, beta=b)
            assert plain.dtype == dt and plain.shape == x.shape
            worst = max(worst, check_levels(plain, lv, dt, (what, basis_name)))
            # / 255, NHWC and the 16-bit outputs of uint8 tiles: the plain output's bits through the library's own cast rules
            unit = be.apply(x.to(dev), basis, alpha=a, beta=b, normalize_to_0_1=True)
            assert same_bits(unit.cpu(), unit_of(plain, dt)), (what, basis_name, "unit")
            for unit_flag in (False, True):
                last = be.apply(nhwc(x).to(dev), basis, alpha=a, beta=b, normalize_to_0_1=unit_flag, channels_last=True)
                assert same_bits(nchw(last), unit if unit_flag else plain), (what, basis_name, "nhwc", unit_flag)
            if dt == torch.uint8:
                for half in (torch.bfloat16, torch.float16):
                    got = be.apply(x.to(dev), basis, alpha=a, beta=b, out_dtype=half)
                    assert same_bits(got.cpu(), plain.cpu().to(half)), (what, basis_name, half)
                    got = be.apply(nhwc(x).to(dev), basis, alpha=a, beta=b, out_dtype=half, normalize_to_0_1=True, channels_last=True)
                    assert same_bits(nchw(got).cpu(), unit_of(plain, dt, half)), (what, basis_name, half, "unit nhwc")
    print(f"{name}: worst figure {worst}")


@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_separate_and_combine_against_the_restatement(dev, be, real, name):
    dt = TORCH_DTYPES[name]
    x8, _ = real
    cases = [(what, tiles.contiguous(), bases) for what, tiles, bases in dn.uint8_separate_cases(x8)]      # (every element type runs the uint8 cases' tiles)
    worst_c = 0.0
    for what, tiles8, bases in cases:
        x = tiles_of(tiles8, dt)
        for basis_name in bases:
            basis = stain_basis(basis_name).to(dev)
            want_c = dn.concentrations(oracle_in(x), basis.cpu().numpy())
            want_i = dn.stain_images(oracle_in(x), basis.cpu().numpy())
            imgs, conc = be.separate(x.to(dev), basis, stains=True, concentrations=True)
            assert imgs.shape == (3,) + tuple(x.shape) and imgs.dtype == dt and conc.shape == x.shape and conc.dtype == torch.float32
            err = float(np.abs(conc.cpu().double().numpy() - want_c).max())
            worst_c = max(worst_c, err)
            print(f"{what} {basis_name} {dt}: max |C - restated| {err:.2e} (bound {CONC_TOL})")
            assert err <= CONC_TOL, (what, basis_name)
            if dt == torch.uint8:      # (the full uint8 rule per stain: tests/test_deconv_cpu.py asserts each one's near-integer share)
                for st in range(3):
                    check_levels(imgs[st], want_i[st], dt, (what, basis_name, "stain image", st))
            else:
                check_levels(imgs, want_i, dt, (what, basis_name, "stain images"))
            if dt == torch.uint8:      # uint8 -> bf16 / f16: the uint8 images' bits through the library's cast rules, plain and / 255, planar and NHWC
                for half in (torch.bfloat16, torch.float16):
                    hi, hc = be.separate(x.to(dev), basis, stains=True, concentrations=True, out_dtype=half)
                    assert hi.dtype == half and same_bits(hi.cpu(), imgs.cpu().to(half)) and same_bits(hc, conc), (what, basis_name, half)
                    hu = be.separate(nhwc(x).to(dev), basis, out_dtype=half, normalize_to_0_1=True, channels_last=True)[0]
                    assert same_bits(hu.permute(0, 1, 4, 2, 3).contiguous().cpu(), unit_of(imgs, dt, half)), (what, basis_name, half, "unit nhwc")
            # each output alone, / 255 and NHWC: the same bits
            assert same_bits(be.separate(x.to(dev), basis, stains=True)[0], imgs) and be.separate(x.to(dev), basis, stains=True)[1] is None
            only_c = be.separate(x.to(dev), basis, stains=False, concentrations=True)
            assert only_c[0] is None and same_bits(only_c[1], conc)
            unit = be.separate(x.to(dev), basis, normalize_to_0_1=True)[0]
            assert same_bits(unit.cpu(), unit_of(imgs, dt)), (what, basis_name, "unit")
            li, lc = be.separate(nhwc(x).to(dev), basis, stains=True, concentrations=True, channels_last=True)
            assert li.shape == (3,) + tuple(nhwc(x).shape) and same_bits(li.permute(0, 1, 4, 2, 3).contiguous(), imgs) and same_bits(nchw(lc), conc)
            # stain image i == apply(alpha = e_i, beta = 0), bit for bit
            n = x.shape[0]
            for s in range(3):
                e = torch.zeros(n, 3, device=dev)
                e[:, s] = 1.0
                assert same_bits(be.apply(x.to(dev), basis, alpha=e, beta=torch.zeros(n, 3, device=dev)), imgs[s]), (what, basis_name, s)
            # combine: float32 against the restatement's levels of the GPU's own concentrations; every other output type is that
            # float32 level through the element type's cast (round to nearest even; float64 exact), bit for bit
            want = dn.combine(conc.cpu().numpy(), basis.cpu().numpy())
            back32 = be.combine(conc, basis, out_dtype=torch.float32)
            check_levels(back32, want, torch.float32, (what, basis_name, "combine"))
            for out_dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
                back = be.combine(conc, basis, out_dtype=out_dt)
                assert same_bits(back.cpu(), back32.cpu().to(out_dt)), (what, basis_name, "combine", out_dt)
                if out_dt in HALF_BOUND:      # float32 within 2.55e-2 followed by round to nearest: within one unit of the format of the restatement's cast
                    d16 = float((back.cpu().double() - torch.from_numpy(np.clip(want, 0, 255)).to(out_dt).double()).abs().max())
                    print(f"{(what, basis_name, 'combine')} {out_dt}: max diff to the restatement's cast {d16} (bound {HALF_BOUND[out_dt]})")
                    assert d16 <= HALF_BOUND[out_dt], (what, basis_name, "combine", out_dt)
                assert same_bits(be.combine(conc, basis, out_dtype=out_dt, normalize_to_0_1=True).cpu(), unit_of(back, out_dt)), out_dt
                assert same_bits(nchw(be.combine(nhwc(conc), basis, out_dtype=out_dt, channels_last=True)), back), out_dt
            back8 = be.combine(conc, basis)
            assert back8.dtype == torch.uint8 and same_bits(back8.cpu(), be.combine(conc, basis, out_dtype=torch.float32).cpu().to(torch.uint8))
            assert same_bits(nchw(be.combine(nhwc(conc), basis, channels_last=True)), back8)
    print(f"{name}: worst concentration error {worst_c:.2e}")


def test_per_tile_bases_from_an_estimate_and_the_anchor_against_macenko_apply(dev, be, real):
    """complement(HE) with alpha = (a_H, a_E, 0), beta = (b_H, b_E, 0) is sx_macenko_apply in own basis with the same HE and factors: the
    residual is dropped exactly.  Compared under the output rule of the element type."""
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    x8, _ = real
    he, full = complement_of(x8, dev)
    n = x8.shape[0]
    a3, b3 = factors(n, dev)
    mac = MacenkoHIP(dev)
    # per-tile bases against the restatement, float32 tiles
    xf = tiles_of(x8, torch.float32)
    got = be.apply(xf.to(dev), full, alpha=a3, beta=b3)
    check_levels(got, dn.apply(xf.numpy(), full.cpu().numpy(), alpha=[dn.ALPHA], beta=[dn.BETA]), torch.float32, "per-tile complement")
    # one basis for the batch == the row repeated; tiles of a batch == the same tiles alone
    one = full[2:3].contiguous()
    assert same_bits(be.apply(xf.to(dev), one, alpha=a3, beta=b3), be.apply(xf.to(dev), one.expand(n, 3, 3).contiguous(), alpha=a3, beta=b3))
    assert same_bits(be.apply(xf.to(dev), one[0], alpha=a3, beta=b3), be.apply(xf.to(dev), one, alpha=a3, beta=b3))
    for i in (0, 4):
        assert same_bits(got[i : i + 1], be.apply(xf[i : i + 1].to(dev), full[i : i + 1].contiguous(), alpha=a3[i : i + 1], beta=b3[i : i + 1]))
    # the anchor
    a3z, b3z = a3.clone(), b3.clone()
    a3z[:, 2] = 0.0
    b3z[:, 2] = 0.0
    for dt in (torch.float32, torch.uint8):
        x = tiles_of(x8, dt).to(dev)
        ours = be.apply(x, full, alpha=a3z, beta=b3z).cpu()
        theirs = mac.apply(x, he, None, alpha=a3z[:, :2].contiguous(), beta=b3z[:, :2].contiguous()).cpu()
        if dt == torch.float32:
            err = float((ours - theirs).abs().max())
            print(f"anchor float32: max |deconv_apply - macenko_apply| {err:.3e} (bound {TOL_255})")
            assert err <= TOL_255
        else:
            levels = dn.apply(x8.numpy(), full.cpu().numpy(), alpha=a3z.cpu().numpy(), beta=b3z.cpu().numpy())
            near = np.abs(levels - np.rint(levels)) <= np.float32(TOL_255)
            o, t = ours.numpy(), theirs.numpy()
            print(f"anchor uint8: near-integer share {near.mean():.3f} (cap {LOOSE_SHARE}), differing pixels {(o != t).sum()} of {o.size}")
            assert near.mean() <= LOOSE_SHARE
            assert np.array_equal(o[~near], t[~near]) and np.abs(o.astype(np.int16) - t.astype(np.int16)).max() <= 1
    # a target basis: stain transfer between two fixed bases
    tgt = stain_basis("hed").to(dev)
    moved = be.apply(xf.to(dev), full, tgt, alpha=a3, beta=b3)
    check_levels(moved, dn.apply(xf.numpy(), full.cpu().numpy(), target=tgt.cpu().numpy(), alpha=[dn.ALPHA], beta=[dn.BETA]), torch.float32, "target basis")
    assert same_bits(moved, be.apply(xf.to(dev), full, tgt.expand(n, 3, 3).contiguous(), alpha=a3, beta=b3))


# ------------------------------------------------------------------------------------------------ 2. identities, bit for bit
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_identities_bit_for_bit(dev, be, lib, real, name):
    dt = TORCH_DTYPES[name]
    x8, _ = real
    x = tiles_of(x8[:3, :, :96, :160].contiguous(), dt).to(dev)      # 15360 pixels: whole packs of every width
    n, _, h, w = x.shape
    basis = stain_basis("hdab").to(dev)
    a, b = factors(n, dev)
    want = be.apply(x, basis, alpha=a, beta=b)
    # NULL factors == explicit ones and zeros
    assert same_bits(be.apply(x, basis), be.apply(x, basis, alpha=torch.ones(n, 3, device=dev), beta=torch.zeros(n, 3, device=dev)))
    # an all-ones mask == the unmasked call
    ones = torch.ones(n, h, w, dtype=torch.uint8, device=dev)
    assert same_bits(be.apply(x, basis, alpha=a, beta=b, masking=(ones, 0.8)), want)
    # aligned == misaligned by one element, for images, output and mask each on their own (vector path vs scalar path)
    assert same_bits(raw_apply(lib, unaligned_copy(x), torch.empty_like(x), basis, alpha=a, beta=b), want)
    assert same_bits(raw_apply(lib, x, unaligned_copy(torch.zeros_like(x)), basis, alpha=a, beta=b), want)
    half = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    half[:, :, w // 3 :] = 1
    masked = be.apply(x, basis, alpha=a, beta=b, masking=(half, 0.8))
    assert same_bits(raw_apply(lib, x, torch.empty_like(x), basis, alpha=a, beta=b, mask=unaligned_copy(half)), masked)
    assert same_bits(raw_apply(lib, unaligned_copy(x), torch.empty_like(x), basis, alpha=a, beta=b, mask=half), masked)
    assert same_bits(raw_apply(lib, x, unaligned_copy(torch.zeros_like(x)), basis, alpha=a, beta=b, mask=half), masked)
    # NHWC: vector (staged stores) vs scalar
    xl = nhwc(x)
    last = raw_apply(lib, xl, torch.empty_like(xl), basis, alpha=a, beta=b, flags=FLAGS["nhwc"])
    assert same_bits(nchw(last), want)
    assert same_bits(raw_apply(lib, unaligned_copy(xl), torch.empty_like(xl), basis, alpha=a, beta=b, flags=FLAGS["nhwc"]), last)
    assert same_bits(raw_apply(lib, xl, unaligned_copy(torch.zeros_like(xl)), basis, alpha=a, beta=b, flags=FLAGS["nhwc"]), last)
    # separate and combine: aligned vs misaligned inputs
    imgs, conc = be.separate(x, basis, stains=True, concentrations=True)
    i2, c2 = be.separate(unaligned_copy(x), basis, stains=True, concentrations=True)
    assert same_bits(i2, imgs) and same_bits(c2, conc)
    assert same_bits(be.combine(unaligned_copy(conc), basis, out_dtype=dt), be.combine(conc, basis, out_dtype=dt))


# ------------------------------------------------------------------------------------------------ 3. round trip and editing
def test_round_trip_and_editing(dev, be, real):
    x8, _ = real
    x = tiles_of(x8[:3, :, :96, :84].contiguous(), torch.float32).to(dev)
    n = x.shape[0]
    for basis_name in NAMES:
        basis = stain_basis(basis_name).to(dev)
        conc = be.separate(x, basis, stains=False, concentrations=True)[1]
        back = be.combine(conc, basis, out_dtype=torch.float32)
        err = float((back - be.apply(x, basis)).abs().max())
        err_in = float((back - (x * 255.0 + 1.0).clamp(0, 255)).abs().max())
        edited = conc.clone()
        edited[:, 2] = 0.0
        keep = torch.tensor([[1.0, 1.0, 0.0]] * n, device=dev)
        err_edit = float((be.combine(edited, basis, out_dtype=torch.float32) - be.apply(x, basis, alpha=keep, beta=torch.zeros(n, 3, device=dev))).abs().max())
        print(f"{basis_name}: |combine(separate(x)) - apply(x)| {err:.3e}, against 255 x + 1 {err_in:.3e}, channel 2 zeroed vs alpha = (1, 1, 0) {err_edit:.3e} (bound {TOL_255})")
        assert err <= TOL_255 and err_in <= TOL_255 and err_edit <= TOL_255, basis_name


# ------------------------------------------------------------------------------------------------ 4. masks
def test_masks(dev, be, real):
    x8, levels = real
    x = x8.to(dev)
    n, _, h, w = x.shape
    basis = stain_basis("hed").to(dev)
    a, b = factors(n, dev)
    rule, _ = tissue_mask(x)
    m = rule.bool().cpu()
    keep = m[:, None].expand(-1, 3, -1, -1)
    got = be.apply(x, basis, alpha=a, beta=b, masking=(rule, 0.8)).cpu()
    assert torch.equal(got[~keep], x8[~keep])      # masked-out pixels: byte-identical
    assert torch.equal(got[keep], be.apply(x, basis, alpha=a, beta=b).cpu()[keep])      # masked-in pixels: the unmasked arithmetic
    assert 0.05 < m.float().mean() < 0.95
    # mask="luminosity" == the explicit mask from tissue_mask()
    assert same_bits(be.apply(x, basis, alpha=a, beta=b, masking=(None, 0.8)).cpu(), got)
    assert same_bits(ColorDeconvolution("hed", device=dev, mask="luminosity").apply(x, a, b).cpu(), got)
    # uint8 under a mask with / 255 and the 16-bit outputs: the plain masked output's bits through the library's cast rules, and the
    # masked-out pixels the background rule (the byte, / 255, cast) spelled out
    unit = be.apply(x, basis, alpha=a, beta=b, masking=(rule, 0.8), normalize_to_0_1=True).cpu()
    assert unit.dtype == torch.float32 and same_bits(unit, unit_of(got, torch.uint8))
    assert torch.equal(unit[~keep], background_expected(x8, True)[~keep])
    for half in (torch.bfloat16, torch.float16):
        for unit_flag in (False, True):
            out = be.apply(x, basis, alpha=a, beta=b, masking=(rule, 0.8), out_dtype=half, normalize_to_0_1=unit_flag).cpu()
            assert same_bits(out, unit_of(got, torch.uint8, half) if unit_flag else got.to(half)), (half, unit_flag)
            assert torch.equal(out[~keep], background_expected(x8, unit_flag, half)[~keep]), (half, unit_flag)
    # float tiles of every width under the mask, plain and / 255: masked-in pixels the unmasked call's bits, masked-out pixels the
    # background rule; NaN / Inf under the mask changes nothing in the masked-in pixels
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        xf = tiles_of(x8, dt).to(dev)
        clean = be.apply(xf, basis, alpha=a, beta=b, masking=(rule, 0.8)).cpu()
        check = dn.apply(oracle_in(xf.cpu()), basis.cpu().numpy(), alpha=[dn.ALPHA], beta=[dn.BETA], mask=m.numpy())
        if dt in (torch.float32, torch.float64):
            check_levels(clean, check, dt, "masked")
        for unit_flag in (False, True):
            out = clean if not unit_flag else be.apply(xf, basis, alpha=a, beta=b, masking=(rule, 0.8), normalize_to_0_1=True).cpu()
            if unit_flag:
                assert same_bits(out, unit_of(clean, dt)), (dt, "unit")
            assert same_bits(out[keep], be.apply(xf, basis, alpha=a, beta=b, normalize_to_0_1=unit_flag).cpu()[keep]), (dt, unit_flag)
            assert same_bits(out[~keep], background_expected(xf.cpu(), unit_flag)[~keep]), (dt, unit_flag)
        dirty = xf.clone()
        dirty[~keep.to(dev)] = float("nan")
        dirty[:, 0][~rule.bool()] = float("inf")
        out = be.apply(dirty, basis, alpha=a, beta=b, masking=(rule, 0.8)).cpu()
        assert same_bits(out[keep], clean[keep]) and not torch.isnan(out[keep].float()).any(), dt
    # a NaN basis row (or target row) copies that tile and leaves its neighbours' bits alone
    rows = basis.expand(n, 3, 3).contiguous()
    bad = rows.clone()
    bad[2, 1, 1] = float("nan")
    ones = torch.ones(n, h, w, dtype=torch.uint8, device=dev)
    for kwargs in ({"basis": bad, "target": None}, {"basis": rows, "target": bad}):
        out = be.apply(x, kwargs["basis"], kwargs["target"], alpha=a, beta=b, masking=(ones, 0.8)).cpu()
        assert torch.equal(out[2], x8[2])
        others = [0, 1, 3, 4, 5]
        assert torch.equal(out[others], be.apply(x, rows, alpha=a, beta=b).cpu()[others])


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_side_stream_graph_replay_and_poisoned_outputs(dev, be, lib, real):
    x8, _ = real
    first = tiles_of(x8[:3, :, :64, :64].contiguous(), torch.float32).to(dev)
    second = tiles_of(x8[3:6, :, 64:128, 64:128].contiguous(), torch.float32).to(dev)
    n, _, h, w = first.shape
    b1, b2 = stain_basis("hed").to(dev).expand(n, 3, 3).contiguous(), torch.stack([stain_basis(k) for k in NAMES]).to(dev)
    a1, be1 = factors(n, dev)
    a2, be2 = a1.flip(1).contiguous(), (be1 * 2).contiguous()
    m1 = torch.ones(n, h, w, dtype=torch.uint8, device=dev)
    m2 = (torch.arange(h * w, device=dev).reshape(1, h, w).expand(n, h, w) % 3 != 0).to(torch.uint8).contiguous()
    want = raw_apply(lib, second, torch.empty_like(second), b2, alpha=a2, beta=be2, mask=m2)
    x, basis, alpha, beta, mask = first.clone(), b1.clone(), a1.clone(), be1.clone(), m1.clone()
    out = poisoned(x.shape, torch.float32, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):      # a side stream, outputs poisoned beforehand
        raw_apply(lib, x, out, basis, alpha=alpha, beta=beta, mask=mask)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    assert same_bits(out, be.apply(first, b1, alpha=a1, beta=be1)) and torch.isfinite(out).all()
    out.view(torch.uint8).fill_(0xA5)
    g = torch.cuda.CUDAGraph()      # (a single kernel node: no parallel branches)
    with torch.cuda.graph(g, stream=s):
        raw_apply(lib, x, out, basis, alpha=alpha, beta=beta, mask=mask)
    for dst, src in ((x, second), (basis, b2), (alpha, a2), (beta, be2), (mask, m2)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want)
    # separate and combine on a side stream into poisoned buffers
    stains, conc = poisoned((3,) + tuple(x.shape), torch.float32, dev), poisoned(x.shape, torch.float32, dev)
    back = poisoned(x.shape, torch.float32, dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        _native.check(lib.sx_deconv_separate(second.data_ptr(), stains.data_ptr(), conc.data_ptr(), f32, n, h, w, b2.data_ptr(), n, 0, _native.stream_ptr(dev)), "sx_deconv_separate", lib)
        _native.check(lib.sx_deconv_combine(conc.data_ptr(), back.data_ptr(), f32, n, h, w, b2.data_ptr(), n, 0, _native.stream_ptr(dev)), "sx_deconv_combine", lib)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    i2, c2 = be.separate(second, b2, stains=True, concentrations=True)
    assert same_bits(stains, i2) and same_bits(conc, c2) and same_bits(back, be.combine(c2, b2, out_dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def test_color_deconvolution_and_hed_augment_end_to_end(dev, be, real):
    x8, levels = real
    x = x8[:4].to(dev)
    cd = ColorDeconvolution("hdab", device=dev)
    a, b = factors(4, dev)
    check_levels(cd.apply(x, a, b), levels["hdab"][:4], torch.uint8, "ColorDeconvolution.apply")
    sep = cd.separate(x, stains=True, concentrations=True)
    assert sep.images.shape == (3, 4, 3, 256, 256) and sep.concentrations.shape == (4, 3, 256, 256) and torch.equal(sep.basis, stain_basis("hdab"))
    assert same_bits(sep.images, be.separate(x, stain_basis("hdab"), stains=True)[0])
    rebuilt = cd.combine(sep.concentrations)
    assert rebuilt.dtype == torch.uint8 and (rebuilt.int() - cd.apply(x).int()).abs().max() <= 1
    # CHW in, CHW out; NHWC through channel_axis=-1
    single = cd.apply(x[0], a[:1], b[:1])
    assert single.shape == (3, 256, 256) and same_bits(single, cd.apply(x, a, b)[0])
    s1 = cd.separate(x[0], concentrations=True)
    assert s1.images.shape == (3, 3, 256, 256) and s1.concentrations.shape == (3, 256, 256)
    last = ColorDeconvolution("hdab", device=dev, channel_axis=-1, normalize_to_0_1=True)
    assert same_bits(nchw(last.apply(nhwc(x), a, b)), ColorDeconvolution("hdab", device=dev, normalize_to_0_1=True).apply(x, a, b))
    # with the factors on the device a Python-level call is the one launch and nothing else: it can be captured (the basis was uploaded once)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        captured = cd.apply(x, a, b)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, cd.apply(x, a, b))
    # HEDAugment: a seeded generator is reproducible, sigma = 0 is apply without factors, CHW in gives CHW out
    aug = HEDAugment(0.05, 0.05, device=dev, generator=torch.Generator().manual_seed(11))
    y1 = aug(x)
    aug.generator.manual_seed(11)
    y2 = aug(x)
    assert y1.dtype == torch.float32 and float(y1.max()) <= 1.0 and same_bits(y1, y2) and not same_bits(y1, aug(x))
    aug.generator.manual_seed(11)
    al, bt = aug.sample_factors(4, dev)
    assert same_bits(y1, ColorDeconvolution("hed", device=dev, normalize_to_0_1=True).apply(x, al, bt))
    still = HEDAugment(0.0, 0.0, device=dev, normalize_to_0_1=False)
    assert same_bits(still(x), ColorDeconvolution("hed", device=dev).apply(x))
    assert still(x[1]).shape == (3, 256, 256) and same_bits(still(x[1]), still(x)[1])
    m = tissue_mask(x)[0]
    masked = HEDAugment(0.1, 0.1, device=dev, normalize_to_0_1=False, mask="luminosity", generator=torch.Generator().manual_seed(3))(x)
    keep = m.bool()[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(masked[~keep], x[~keep])
    # ... and with the module's default normalisation (/ 255, float32): the same draw's bits through / 255, glass the byte / 255
    by_default = HEDAugment(0.1, 0.1, device=dev, mask="luminosity", generator=torch.Generator().manual_seed(3))(x)
    assert by_default.dtype == torch.float32 and same_bits(by_default.cpu(), unit_of(masked, torch.uint8))
    assert torch.equal(by_default[~keep].cpu(), (x8[:4].float() / 255.0)[~keep.cpu()]) and not torch.equal(by_default[keep].cpu(), (x8[:4].float() / 255.0)[keep.cpu()])
