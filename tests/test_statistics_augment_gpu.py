"""Statistics-space augmentation on the GPU: the apply pass with a target per tile (include/stainx_hip.h: sx_reinhard_apply_targets /
_targets_masked) bit for bit against the given-statistics calls and against the CPU oracle tile by tile; the integer moments of the
concentrations (sx_deconv_moments / _moments_masked) exactly against the rule restated in tests/_statistics_numpy.py on what
sx_deconv_separate writes; ``ColorDeconvolution.match`` and ``StatisticsAugment.forward`` against the calls they are composed of.

Shapes.  The LAB apply pass takes packs of four pixels where the tile size and the pointers allow it, single elements otherwise:
  96 x 96   = 9216 pixels, five tiles: the pack path on an aligned base, nine work items per tile; the scalar path one element behind it
  37 x 29   = 1073 pixels, three tiles: odd, the scalar path wherever it lies, two work items per tile (the last one partial)
A work item of deconv_moments_kernel is 8192 pixels of one tile (tests/test_quantify_gpu.py lists the pack sets per element type):
  160 x 112 = 17920: 2.19 work items, the last one partial;   77 x 79 = 6083: odd, the scalar path, one partial work item."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import (ColorDeconvolution, ColorStatistics, ConcentrationStatistics, Macenko, Reinhard, StatisticsAugment, StatisticsDistribution, _native, stain_basis,
                        synth)
from tests import _masked_numpy as mn
from tests import _statistics_numpy as sn
from tests.conftest import TORCH_DTYPES
from tests.test_per_tile_gpu import assert_reinhard_close, mixed_batch, oracle_cast, oracle_input
from tests.test_statistics_augment_cpu import lab_targets

pytestmark = pytest.mark.gpu

DTYPES = ["u8", "f32", "bf16", "f16", "f64"]
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lab_be(dev):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    return ReinhardHIP(dev)


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import DeconvHIP

    return DeconvHIP(dev)


@pytest.fixture(scope="module")
def real():
    """The six 256 x 256 real crops (uint8, CPU): never changed."""
    return mn.real_crops(256)


@pytest.fixture(scope="module")
def targets():
    """(5, 3) float32 each, CPU: the per-tile LAB statistics of five synthetic H&E tiles (computed once, never changed)."""
    mean, std = lab_targets()
    return torch.from_numpy(mean), torch.from_numpy(std)


def aligned_copy(x: torch.Tensor, dev) -> torch.Tensor:
    out = torch.empty(x.shape, dtype=x.dtype, device=dev)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return out


def unaligned_copy(x: torch.Tensor, dev) -> torch.Tensor:
    """The same values, dense, one element behind an aligned address (a view into a buffer one element longer)."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def lab_cases(dt: torch.dtype, dev):
    """(what, tiles on the CPU, tiles on the device) for the two shapes, each on an aligned base and one element behind one."""
    x8 = mixed_batch()[0]
    for what, tiles8 in (("5x96x96", x8), ("3x37x29", x8[:3, :, 30:67, 40:69].contiguous())):
        src = synth.as_dtype(tiles8, dt)
        yield what + " aligned", src, aligned_copy(src, dev)
        yield what + " unaligned", src, unaligned_copy(src, dev)


def half_mask(n: int, h: int, w: int, dev) -> torch.Tensor:
    """(N, H, W) uint8: a different pattern per tile, about half of the pixels in; no run of four is all in or all out everywhere."""
    g = torch.Generator().manual_seed(77)
    return (torch.rand((n, h, w), generator=g) < 0.5).to(torch.uint8).to(dev)


# ------------------------------------------------------------------------------------------------ LAB: bits
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("name", DTYPES)
def test_apply_targets_bits(dev, lab_be, targets, name, masked):
    dt = TORCH_DTYPES[name]
    for what, _, x in lab_cases(dt, dev):
        n, _, h, w = x.shape
        mask = half_mask(n, h, w, dev) if masked else None
        tm, ts = targets[0][:n].to(dev), targets[1][:n].to(dev)
        if masked:
            sm, ss, _ = lab_be.masked_statistics(x, mask, 0.8, per_tile=True)
            stats = lambda *a: lab_be.apply_statistics_masked(*a, mask, 0.8)      # noqa: E731
            tgts = lambda *a: lab_be.apply_targets_masked(*a, mask, 0.8)      # noqa: E731
        else:
            sm, ss = lab_be.tile_statistics(x)
            stats, tgts = lab_be.apply_statistics, lab_be.apply_targets
        assert torch.isfinite(sm).all() and torch.isfinite(ss).all()
        # one target row: the bits of the given-statistics call, with per-tile and with one row of source statistics
        for rows in (slice(0, n), slice(1, 2)):
            want = stats(x, sm[rows], ss[rows], tm[2], ts[2])
            assert torch.equal(tgts(x, sm[rows], ss[rows], tm[2:3], ts[2:3]), want), (what, name, rows)
            assert torch.equal(tgts(x, sm[rows], ss[rows], tm[2], ts[2]), want), (what, name, rows, "(3,)")
        # a target per tile: tile t is the one-tile call with rows t -- and the given-statistics call with target t
        got = tgts(x, sm, ss, tm, ts)
        assert got.dtype == dt and got.shape == x.shape
        for t in range(n):
            if masked:
                one = lab_be.apply_targets_masked(x[t:t + 1], sm[t:t + 1], ss[t:t + 1], tm[t:t + 1], ts[t:t + 1], mask[t:t + 1], 0.8)
            else:
                one = lab_be.apply_targets(x[t:t + 1], sm[t:t + 1], ss[t:t + 1], tm[t:t + 1], ts[t:t + 1])
            assert torch.equal(got[t:t + 1], one), (what, name, t)
            assert torch.equal(got[t], stats(x, sm, ss, tm[t], ts[t])[t]), (what, name, t, "against the given-statistics call")
        assert not torch.equal(got[0], stats(x, sm, ss, tm[1], ts[1])[0])      # (the targets differ: so do the tiles)
        if masked:      # glass keeps its bits, tissue gets the unmasked call's
            out_of = (mask == 0).unsqueeze(1).expand_as(x)
            assert torch.equal(got[out_of], x[out_of]), (what, name)
            plain = lab_be.apply_targets(x, sm, ss, tm, ts)
            assert torch.equal(got[~out_of], plain[~out_of]), (what, name)
        # a NaN in any of the four arrays copies exactly that tile, bit for bit
        for which in range(4):
            rows4 = [sm.clone(), ss.clone(), tm.clone(), ts.clone()]
            rows4[which][1, which % 3] = NAN
            left = tgts(x, *rows4)
            assert torch.equal(left[1], x[1]), (what, name, which)
            keep = [t for t in range(n) if t != 1]
            assert torch.equal(left[keep], got[keep]), (what, name, which)
        # one NaN row for the whole batch leaves every tile
        assert torch.equal(tgts(x, sm, ss, torch.full((1, 3), NAN, device=dev), ts[:1]), x), (what, name)


def test_given_statistics_calls_keep_their_behaviour_on_nan_rows(dev, lab_be, targets):
    """The existing unmasked entry point does NOT copy a tile whose row holds a NaN (only the new calls do)."""
    x = aligned_copy(synth.as_dtype(mixed_batch()[0], torch.float32), dev)
    sm, ss = lab_be.tile_statistics(x)
    sm[1, 0] = NAN
    old = lab_be.apply_statistics(x, sm, ss, targets[0][0], targets[1][0])
    new = lab_be.apply_targets(x, sm, ss, targets[0][:1], targets[1][:1])
    assert not torch.equal(old[1], x[1]) and torch.equal(new[1], x[1])
    assert torch.equal(old[[0, 2, 3, 4]], new[[0, 2, 3, 4]])


# ------------------------------------------------------------------------------------------------ LAB: against the oracle, tile by tile
@pytest.mark.parametrize("name", DTYPES)
def test_apply_targets_against_the_oracle(dev, targets, name):
    """The three rules of ``assert_reinhard_close`` (tests/test_per_tile_gpu.py): float32 1e-4; uint8 at most one level with a share below
    5e-3; 16-bit floats 2^-8 with a share below 2e-2.  A DEVIATION for float64, which that helper sends down the 16-bit branch: its
    maximum is held to float32's 1e-4 (tighter than 2^-8) and the share rule is NOT applied -- the oracle is float32 arithmetic cast to
    float64, so an unquantised float64 output differs from it in the last bits of nearly every element (share measured 0.84, maximum
    6.6e-7), which says nothing about the kernel."""
    dt = TORCH_DTYPES[name]
    r = Reinhard(device=dev, backend="torch_hip")
    for what, src, x in lab_cases(dt, dev):
        n = x.shape[0]
        tm, ts = targets[0][:n], targets[1][:n]
        xin = oracle_input(src)
        want = oracle_cast(np.concatenate([so.reinhard_transform(xin[i:i + 1], tm[i].numpy(), ts[i].numpy()) for i in range(n)]), dt)
        got = r.apply(x, r.estimate(x), target=(tm.to(dev), ts.to(dev)))      # (no fit)
        assert got.dtype == dt
        if dt == torch.float64:      # (see the docstring: float32's rule, 1e-4, without the share rule of the quantised outputs)
            worst = (got.cpu() - want).abs().max().item()
            print(f"reinhard targets {what} float64: max |diff| {worst:.3e}")
            assert worst <= 1e-4, (what, worst)
        else:
            assert_reinhard_close(got.cpu(), want, f"targets {what}")


# ------------------------------------------------------------------------------------------------ moments: exact
def separated(be, x: torch.Tensor, basis: torch.Tensor, channels_last: bool = False) -> np.ndarray:
    conc = be.separate(x, basis, stains=False, concentrations=True, channels_last=channels_last)[1]
    return (conc.permute(0, 3, 1, 2) if channels_last else conc).contiguous().cpu().numpy()


def same(got, want, what) -> None:
    sums, squares, pixels = (t.cpu().numpy() for t in got[:3])
    assert sums.dtype == np.int64 and squares.dtype == np.int64 and pixels.dtype == np.int64, what
    assert sums.shape == want[0].shape and squares.shape == want[1].shape and pixels.shape == want[2].shape, what
    assert np.array_equal(pixels, want[2]), (what, "pixels", pixels, want[2])
    assert np.array_equal(sums, want[0]), (what, "sums", sums, want[0])
    assert np.array_equal(squares, want[1]), (what, "squares", squares, want[1])


@pytest.mark.parametrize("name", DTYPES)
def test_moments_are_the_rule_on_the_separations_bits(dev, be, real, name):
    dt = TORCH_DTYPES[name]
    tiles_basis = Macenko(device=dev).estimate(real[:3].to(dev)).complement().contiguous()
    for what, tiles8 in (("160x112", real[:3, :, :160, :112].contiguous()), ("77x79", real[:3, :, 11:88, 5:84].contiguous())):
        x = (tiles8 if dt == torch.uint8 else (tiles8.float() / 255.0).to(dt)).to(dev)
        n, _, h, w = x.shape
        for basis_name, basis in (("hed", stain_basis("hed").to(dev)), ("tiles", tiles_basis)):
            conc = separated(be, x, basis)
            want = sn.moments_of(conc)
            got = be.moments(x, basis)
            same(got, want, (what, name, basis_name))
            assert int(want[2].sum()) == n * h * w and (want[1] > 0).all()
            quant = be.quantify(x, basis)
            assert torch.equal(got[0], quant[1]) and torch.equal(got[2], quant[2]), (what, name, basis_name, "quantify's sums and pixels")
            same(be.moments(x, basis, per_tile=False), sn.pooled(*want), (what, name, basis_name, "pooled"))
            xl = x.permute(0, 2, 3, 1).contiguous()
            same(be.moments(xl, basis, channels_last=True), sn.moments_of(separated(be, xl, basis, True)), (what, name, basis_name, "nhwc"))
            same(be.moments(xl, basis, channels_last=True), want, (what, name, basis_name, "nhwc against planar"))
            ones = torch.ones((n, h, w), dtype=torch.uint8, device=dev)
            same(be.moments(x, basis, masking=(ones, 0.8)), want, (what, name, basis_name, "all-ones mask"))
            half = half_mask(n, h, w, dev)
            kept = sn.moments_of(conc, keep=half.cpu().numpy().astype(bool))
            same(be.moments(x, basis, masking=(half, 0.8)), kept, (what, name, basis_name, "half mask"))
            same(be.moments(x, basis, per_tile=False, masking=(half, 0.8)), sn.pooled(*kept), (what, name, basis_name, "half mask, pooled"))
            # one element behind an aligned address: the scalar path, the same integers
            flat = torch.empty(x.numel() + 1, dtype=dt, device=dev)
            view = flat[1:].view(x.shape)
            view.copy_(x)
            assert view.data_ptr() % 16 != 0
            same(be.moments(view, basis), want, (what, name, basis_name, "misaligned"))
        # a NaN basis row counts nothing
        bad = tiles_basis.clone()
        bad[1, 2, 0] = NAN
        got = be.moments(x, bad)
        want = sn.moments_of(separated(be, x, tiles_basis))
        for part, w_part in zip(got, want):
            assert part[1].eq(0).all() and np.array_equal(part[[0, 2]].cpu().numpy(), w_part[[0, 2]]), (what, name, "NaN basis row")


def test_moments_clamp_and_uncounted_pixels(dev, be):
    """float32 tiles with zeros and values near 1e-30 (optical density ln 240 in every channel) under a nearly singular basis: concentrations
    beyond +-64, so the clamp of u_s is taken; NaN / Inf / below-the-pole elements are not counted."""
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 77, 79), generator=g, dtype=torch.float32)
    x[0, :, :20] = 0.0
    x[1, :, 30:50] = 1e-30
    x[0, 0, 40, 3], x[0, 1, 41, 4], x[1, 2, 5, 5], x[1, 0, 6, 6] = NAN, float("inf"), -1.0, -2.0 / 255.0      # (255 x + 1 < 0: no logarithm)
    hed = stain_basis("hed")
    near = hed.clone()
    near[:, 1] = hed[:, 0] + 0.02 * hed[:, 1]
    near[:, 1] /= near[:, 1].norm()
    xd = x.to(dev)
    for what, basis in (("hed", hed.to(dev)), ("nearly singular", near.to(dev))):
        conc = separated(be, xd, basis)
        want = sn.moments_of(conc)
        same(be.moments(xd, basis), want, what)
        assert want[2].tolist() == [77 * 79 - 2, 77 * 79 - 2], (what, want[2])
        clamped = int((np.abs(sn.qn.terms_of(np.where(np.isfinite(conc), conc, 0.0))) > sn.CLAMP).sum())
        print(f"{what}: {clamped} terms beyond the clamp, largest |C| {np.nanmax(np.abs(np.where(np.isfinite(conc), conc, np.nan))):.1f}")
        assert (clamped > 1000) == (what == "nearly singular"), (what, clamped)


def test_estimate_pools_exactly_and_feeds_fit(dev, real):
    cd = ColorDeconvolution("hed", device=dev)
    a, b = real[:4].to(dev), real[4:].to(dev)
    sa, sb = cd.estimate(a), cd.estimate(b)
    assert isinstance(sa, ConcentrationStatistics) and tuple(sa.sums.shape) == (4, 3) and tuple(sa.pixels.shape) == (4,)
    whole = cd.estimate(real.to(dev), pooled=True)
    both = ConcentrationStatistics.pool(sa, sb)
    assert all(torch.equal(p, q) for p, q in zip(both, whole))
    again = cd.estimate(a)
    assert all(torch.equal(p, q) for p, q in zip(sa, again))      # integers: the same run to run
    conc64 = sn.dn.concentrations(real.numpy(), stain_basis("hed").numpy()).reshape(6, 3, -1)
    every = ConcentrationStatistics(*(torch.cat([p, q]) for p, q in zip(sa, sb)))
    mean_err = float(np.abs(every.mean().cpu().numpy() - conc64.mean(-1)).max())
    std_err = float(np.abs(every.std().cpu().numpy() - conc64.std(-1, ddof=1)).max())
    print(f"estimate against float64 on the real crops: max |mean - mean64| {mean_err:.3e}, max |std - std64| {std_err:.3e}")
    # (the mean: quantify's bound.  The std: every value is within CONC_TOL of float64, so the centred values within 2 CONC_TOL and the
    # root mean square with them; the terms' rounding adds 2^-17, the floor of the squares less than 2^-24 on C^2)
    assert mean_err <= sn.qn.CONC_TOL + 2.0**-17 and std_err <= 2.0 * sn.qn.CONC_TOL + 2.0**-16
    d = StatisticsDistribution.fit(sa, sb)
    m, s = sn.mean_std(*(t.cpu().numpy() for t in every))
    for got, want in zip(d, sn.fit_distribution(m, s)):      # (float64 on the device against float64 in numpy, rounded to float32)
        assert np.allclose(got.numpy(), want, rtol=1e-6, atol=0.0)
    single = cd.estimate(real[0].to(dev))      # CHW: one set
    assert tuple(single.sums.shape) == (1, 3) and torch.equal(single.sums[0], sa.sums[0])


# ------------------------------------------------------------------------------------------------ match and forward
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_match_is_apply_with_the_restated_factors(dev, real, name):
    dt = TORCH_DTYPES[name]
    tiles8 = real[:4, :, :96, :84].contiguous()
    x = (tiles8 if dt == torch.uint8 else (tiles8.float() / 255.0).to(dt)).to(dev)
    cd = ColorDeconvolution("hed", device=dev, normalize_to_0_1=True)
    src = cd.estimate(x)
    sm, ss = src.mean(), src.std()
    tm = torch.tensor([[0.5, 0.3, 0.1], [0.2, 0.2, 0.2], [NAN, 0.3, 0.1], [0.4, 0.1, 0.0]], dtype=torch.float32, device=dev)
    ts = torch.tensor([[0.2, 0.001, 0.9], [0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.3, 0.2, 0.1]], dtype=torch.float32, device=dev)
    mask = half_mask(4, 96, 84, dev)
    for gain in ((0.1, 2.5), (0.8, 1.25)):
        alpha, beta = sn.match_factors(sm.cpu().numpy(), ss.cpu().numpy(), tm.cpu().numpy(), ts.cpu().numpy(), 4, gain)
        assert (alpha[2] == 1.0).all() and (beta[2] == 0.0).all() and len(set(alpha.ravel().tolist())) > (4 if gain == (0.1, 2.5) else 2)
        a, b = torch.from_numpy(alpha).to(dev), torch.from_numpy(beta).to(dev)
        assert torch.equal(cd.match(x, src, (tm, ts), gain_range=gain), cd.apply(x, a, b)), (name, gain)
        assert torch.equal(cd.match(x, (sm, ss), (tm, ts), gain_range=gain, mask=mask), cd.apply(x, a, b, mask=mask)), (name, gain, "masked")
    # a zero standard deviation in the source row: the identity factors for the tile
    flat = ss.clone()
    flat[0, 1] = 0.0
    alpha, beta = sn.match_factors(sm.cpu().numpy(), flat.cpu().numpy(), tm[0].cpu().numpy(), ts[0].cpu().numpy(), 4)
    assert (alpha[0] == 1.0).all() and (beta[0] == 0.0).all()
    assert torch.equal(cd.match(x, (sm, flat), (tm[0], ts[0])), cd.apply(x, torch.from_numpy(alpha).to(dev), torch.from_numpy(beta).to(dev)))


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_forward_is_the_composed_calls(dev, targets, name):
    dt = TORCH_DTYPES[name]
    x = aligned_copy(synth.as_dtype(mixed_batch()[0], dt), dev)
    n, _, h, w = x.shape
    mask = half_mask(n, h, w, dev)
    tm, ts = targets[0].to(dev), targets[1].to(dev)
    d_lab = StatisticsDistribution.fit(ColorStatistics(*targets))
    # LAB: estimate, the clamp of the target std on the device, one apply launch with a target per tile
    lab = StatisticsAugment(d_lab, "lab", gain_range=(0.5, 1.5), device=dev)
    r = Reinhard(device=dev, backend="torch_hip")
    for m in (None, mask):
        own = r.estimate(x, mask=m)
        clamped = torch.minimum(torch.maximum(ts, 0.5 * own.std), 1.5 * own.std)
        assert not torch.equal(clamped, ts)      # (the noise tiles: the clamp is taken)
        got = lab(x, targets=(tm, ts), mask=m)
        assert got.dtype == dt and torch.equal(got, r.apply(x, own, m, target=(tm, clamped))), (name, m is None)
        if m is not None:      # glass keeps its bits
            out_of = (m == 0).unsqueeze(1).expand_as(x)
            assert torch.equal(got[out_of], x[out_of]) and not torch.equal(got, x)
    # zero spreads: the centres are every tile's target (gain range wide enough that the clamp is not taken on these tiles)
    flat = StatisticsAugment(StatisticsDistribution(d_lab.mean_center, torch.zeros(3), d_lab.std_center, torch.zeros(3)), "lab", gain_range=(1e-3, 1e3), device=dev)
    own = r.estimate(x)
    ratio = d_lab.std_center.to(dev) / own.std
    assert 1e-3 < float(ratio.min()) and float(ratio.max()) < 1e3
    assert torch.equal(flat(x), r.apply(x, own, target=(d_lab.mean_center, d_lab.std_center)))
    assert flat(x[0]).shape == x[0].shape      # (CHW in, CHW out)
    # HED: estimate, then match; under a mask apply's masked copy
    cd = ColorDeconvolution("hed", device=dev, normalize_to_0_1=True)
    src = cd.estimate(x)
    d_hed = StatisticsDistribution.fit(src)
    hed = StatisticsAugment(d_hed, "hed", device=dev)
    hm, hs = src.mean().float().flip(0).contiguous(), src.std().float().flip(0).contiguous()      # (tile t gets the statistics of tile n - 1 - t)
    assert torch.equal(hed(x, targets=(hm, hs)), cd.match(x, src, (hm, hs)))
    src_m = cd.estimate(x, mask=mask)
    got = hed(x, targets=(hm, hs), mask=mask)
    assert torch.equal(got, cd.match(x, src_m, (hm, hs), mask=mask))
    alpha, beta = sn.match_factors(src_m.mean().cpu().numpy(), src_m.std().cpu().numpy(), hm.cpu().numpy(), hs.cpu().numpy(), n)
    assert torch.equal(got, cd.apply(x, torch.from_numpy(alpha).to(dev), torch.from_numpy(beta).to(dev), mask=mask))
    rule = StatisticsAugment(d_hed, "hed", mask="luminosity", device=dev)
    tissue = ColorDeconvolution("hed", device=dev, normalize_to_0_1=True, mask="luminosity")
    assert torch.equal(rule(x, targets=(hm, hs)), tissue.match(x, tissue.estimate(x), (hm, hs)))
    # drawn targets: the module's own draw, reproduced from its generator's seed
    for space, dist in (("lab", d_lab), ("hed", d_hed)):
        drawn = StatisticsAugment(dist, space, kind="laplace", p=0.6, generator=torch.Generator().manual_seed(9), device=dev)
        twin = StatisticsAugment(dist, space, kind="laplace", p=0.6, generator=torch.Generator().manual_seed(9), device=dev)
        own = r.estimate(x) if space == "lab" else (src.mean(), src.std())
        want_targets = twin.sample_targets(n, dev, own=own)
        assert torch.equal(drawn(x), twin(x, targets=want_targets)), space


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_a_tile_of_one_pixel_passes_through(dev, name):
    dt = TORCH_DTYPES[name]
    x = synth.as_dtype(torch.tensor([[[[200]], [[120]], [[180]]], [[[90]], [[60]], [[140]]]], dtype=torch.uint8), dt).to(dev)
    d = StatisticsDistribution(torch.tensor([150.0, 140.0, 120.0]), torch.ones(3), torch.tensor([30.0, 10.0, 8.0]), torch.ones(3))
    assert torch.equal(StatisticsAugment(d, "lab", device=dev)(x), x)      # no statistics: the bits of the input
    hed = StatisticsAugment(StatisticsDistribution(torch.tensor([0.4, 0.2, 0.1]), torch.ones(3) * 0.1, torch.tensor([0.2, 0.1, 0.1]), torch.ones(3) * 0.01), "hed", device=dev)
    assert torch.equal(hed(x), hed.deconv.apply(x))      # the identity factors: apply's round trip
    # a mask that leaves a tile fewer than two pixels
    y = aligned_copy(synth.as_dtype(mixed_batch()[0][:2], dt), dev)
    mask = torch.ones((2, 96, 96), dtype=torch.uint8, device=dev)
    mask[1] = 0
    mask[1, 4, 4] = 1
    out = StatisticsAugment(d, "lab", device=dev)(y, mask=mask)
    assert torch.equal(out[1], y[1]) and not torch.equal(out[0], y[0])


@pytest.mark.parametrize("space", ["lab", "hed"])
def test_a_captured_call_replays_with_new_targets(dev, targets, real, space):
    x = aligned_copy(synth.as_dtype(mixed_batch()[0], torch.float32), dev)
    n = x.shape[0]
    if space == "lab":
        first, second = (targets[0].to(dev), targets[1].to(dev)), (targets[0].flip(0).to(dev), (targets[1].flip(0) * 1.1).to(dev))
        dist = StatisticsDistribution.fit(ColorStatistics(*targets))
    else:
        src = ColorDeconvolution("hed", device=dev).estimate(x)
        first = (src.mean().float().flip(0).contiguous(), src.std().float().flip(0).contiguous())
        second = (first[0] * 1.2 + 0.05, first[1] * 0.7)
        dist = StatisticsDistribution.fit(src)
    aug = StatisticsAugment(dist, space, device=dev)
    want_first, want_second = aug(x, targets=first), aug(x, targets=second)
    assert not torch.equal(want_first, want_second)
    mean_buf, std_buf = first[0].clone(), first[1].clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):      # (warm-up on the capture stream: its workspaces exist before the capture)
        aug(x, targets=(mean_buf, std_buf))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = aug(x, targets=(mean_buf, std_buf))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_first), space
    mean_buf.copy_(second[0])
    std_buf.copy_(second[1])
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, want_second), space
