"""Stain quantification on the GPU (include/stainx_hip.h: sx_deconv_quantify / _quantify_masked): bit for bit against the binning rule
applied to what sx_deconv_separate writes (tests/_quantify_numpy.py), against the float64 restatement of the concentrations, pooling,
masks, non-finite pixels, the figures of ``StainHistograms`` on device results, and a captured graph.

Shapes.  A work item of deconv_quantify_kernel is kQuantPixels = 8192 pixels of one tile for every pack width, swept by 256 threads in
pack sets of 256 V pixels (V = 1 on the scalar path, 2 / 4 / 8 / 16 for float64 / float32 / 16-bit / uint8 packs):
  33 x 37   = 1221 pixels: odd, the scalar path, one work item of 4.8 sweeps
  67 x 65   = 4355: the scalar path, one work item, 17.01 sweeps (a last sweep of 3 pixels)
  131 x 67  = 8777: the scalar path, 1.07 work items
  96 x 84   = 8064: 0.98 work items -- 15.75 pack sets of float64, 7.9 of float32, 3.9 of 16-bit, 1.97 of uint8 (each partial)
  160 x 112 = 17920: 2.19 work items; the last one holds 1536 pixels: 3 / 1.5 / 0.75 / 0.375 pack sets
  256 x 256 = 65536: the real crops, 8 whole work items
  296 x 256 = 75776: a crop with the first 40 rows of the next one below it, 9.25 work items -- more than two, the last one partial
              (2048 pixels: whole pack sets of float64 / float32 / 16-bit, half a set of uint8)

The float64 test prints the near-edge share beside its cap, the number of values outside their certain bin and the largest mean error
beside its bound; test 1 prints how many values the end bins hold."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import ColorDeconvolution, Macenko, StainHistograms, _native, stain_basis, tissue_mask
from tests import _masked_numpy as mn
from tests import _quantify_numpy as qn
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu

NAMES = ("hed", "he", "hdab")
CONC_TOL = qn.CONC_TOL
WORDS = 772
DEFAULT, FINE = (5, 64), (8, 32)      # [-2, 6) in bins of 1/32: both end bins saturate on the real crops; [-1/8, 7/8) in bins of 1/256: 20-40 % in the end bins
SMALL = {"33x37": (3, 33, 37), "67x65": (2, 67, 65), "131x67": (2, 131, 67), "96x84": (3, 96, 84), "160x112": (2, 160, 112)}


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
    """The six 256 x 256 real crops (uint8, CPU): never changed."""
    return mn.real_crops(256)


@pytest.fixture(scope="module")
def per_tile(real, dev):
    """(6, 3, 3): the complemented per-tile Macenko estimates of the crops, on the device."""
    return Macenko(device=dev).estimate(real.to(dev)).complement().contiguous()


def tiles_of(x8: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    return x8 if dt == torch.uint8 else (x8.float() / 255.0).to(dt)


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def long_tiles(x8: torch.Tensor) -> torch.Tensor:
    """(2, 3, 296, 256): crop i with the first 40 rows of crop i + 1 below it."""
    return torch.stack([torch.cat([x8[i], x8[i + 1][:, :40]], dim=1) for i in range(2)]).contiguous()


def separated(be, x: torch.Tensor, basis: torch.Tensor, channels_last: bool = False) -> np.ndarray:
    """(N, 3, H, W) float32 on the CPU: what sx_deconv_separate writes for ``x`` (on the device, in the call's own layout)."""
    conc = be.separate(x, basis, stains=False, concentrations=True, channels_last=channels_last)[1]
    return (conc.permute(0, 3, 1, 2) if channels_last else conc).contiguous().cpu().numpy()


def same(got, want, what) -> None:
    counts, sums, pixels = (t.cpu().numpy() for t in got[:3])
    assert counts.dtype == np.int64 and sums.dtype == np.int64 and pixels.dtype == np.int64, what
    assert counts.shape == want[0].shape and sums.shape == want[1].shape and pixels.shape == want[2].shape, what
    assert np.array_equal(pixels, want[2]), (what, "pixels", pixels, want[2])
    assert np.array_equal(counts, want[0]), (what, "counts", int(np.abs(counts - want[0]).sum()))
    assert np.array_equal(sums, want[1]), (what, "sums", sums, want[1])


def poisoned_rows(sets: int, dev) -> torch.Tensor:
    t = torch.empty((sets, WORDS), dtype=torch.int64, device=dev)
    t.view(torch.uint8).fill_(0xA5)
    return t


def unaligned_copy(x: torch.Tensor) -> torch.Tensor:
    """The same values, dense, one element behind an aligned address."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    return view


def raw_quantify(lib, x, basis, k, z, per_tile_flag=True, mask=None, flags=0, out=None):
    """The C ABI on caller-owned buffers; returns (counts, sums, pixels) views of ``out``."""
    last = bool(flags & _native.MACENKO_CHANNELS_LAST)
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if last else (x.shape[0], x.shape[2], x.shape[3])
    nb = 1 if basis.dim() == 2 else basis.shape[0]
    sets = n if per_tile_flag else 1
    out = poisoned_rows(sets, x.device) if out is None else out
    code, stream = _native.DTYPE_CODES[x.dtype], _native.stream_ptr(x.device)
    if mask is None:
        rc = lib.sx_deconv_quantify(x.data_ptr(), code, n, h, w, basis.data_ptr(), nb, k, z, int(per_tile_flag), out.data_ptr(), flags, stream)
    else:
        rc = lib.sx_deconv_quantify_masked(x.data_ptr(), code, n, h, w, basis.data_ptr(), nb, k, z, int(per_tile_flag), out.data_ptr(), mask.data_ptr(), flags, stream)
    _native.check(rc, "sx_deconv_quantify", lib)
    return out[:, :768].view(sets, 3, 256), out[:, 768:771], out[:, 771]


# ------------------------------------------------------------------------------------------------ 1. bit for bit against the separation
@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_quantify_is_the_binning_rule_on_the_separations_bits(dev, be, real, per_tile, name):
    dt = TORCH_DTYPES[name]
    cases = [("real", real, NAMES + ("tiles",), (DEFAULT, FINE)), ("296x256", long_tiles(real), ("hdab", "tiles"), (DEFAULT,))]
    for shape_name, (n, h, w) in SMALL.items():
        cases.append((shape_name, real[:n, :, 11 : 11 + h, 5 : 5 + w].contiguous(), ("hdab", "tiles"), (DEFAULT,)))
    end_bins = {DEFAULT: [0, 0], FINE: [0, 0]}
    for what, tiles8, bases, binnings in cases:
        x = tiles_of(tiles8, dt).to(dev)
        n = x.shape[0]
        for basis_name in bases:
            basis = per_tile[:n].contiguous() if basis_name == "tiles" else stain_basis(basis_name).to(dev)
            for last in (False, True):
                xin = nhwc(x) if last else x
                conc = separated(be, xin, basis, last)
                for k, z in binnings:
                    want = qn.histogram_of(conc, k, z)
                    got = be.quantify(xin, basis, bin_log2=k, zero_bin=z, channels_last=last)
                    same(got, want, (what, name, basis_name, last, k, z))
                    assert int(want[2].sum()) == x.shape[0] * x.shape[2] * x.shape[3]
                    if what == "real" and not last and basis_name != "tiles":
                        low, high = int(want[0][:, :, 0].sum()), int(want[0][:, :, 255].sum())
                        print(f"{name} {basis_name} k={k} z={z}: end bins hold {low} + {high} of {int(want[0].sum())} values")
                        end_bins[(k, z)][0] += low
                        end_bins[(k, z)][1] += high
    assert all(low > 0 and high > 0 for low, high in end_bins.values()), ("both binnings must saturate at both ends on the real crops", end_bins)


@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16", "f64"])
def test_raw_calls_on_misaligned_views_and_poisoned_buffers(dev, be, lib, real, per_tile, name):
    dt = TORCH_DTYPES[name]
    for what, tiles8 in (("160x112", real[:2, :, :160, :112].contiguous()), ("96x84", real[:3, :, 7:103, 9:93].contiguous())):
        x = tiles_of(tiles8, dt).to(dev)
        n = x.shape[0]
        for basis in (stain_basis("hed").to(dev), per_tile[:n].contiguous()):
            want = qn.histogram_of(separated(be, x, basis), *DEFAULT)
            same(raw_quantify(lib, x, basis, *DEFAULT), want, (what, name, "aligned"))      # every word of the poisoned buffer is overwritten, zero bins included
            same(raw_quantify(lib, unaligned_copy(x), basis, *DEFAULT), want, (what, name, "misaligned: the scalar path"))
            same(raw_quantify(lib, unaligned_copy(nhwc(x)), basis, *DEFAULT, flags=_native.MACENKO_CHANNELS_LAST), want, (what, name, "misaligned nhwc"))
            same(raw_quantify(lib, x, basis, *DEFAULT, per_tile_flag=False), qn.pooled(*want), (what, name, "pooled"))
            ones = torch.ones((n,) + tuple(x.shape[2:]), dtype=torch.uint8, device=dev)
            same(raw_quantify(lib, x, basis, *DEFAULT, mask=ones), want, (what, name, "all-ones mask"))
            same(raw_quantify(lib, x, basis, *DEFAULT, flags=_native.MACENKO_CLASSIC), want, (what, name, "classic is a no-op"))


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("name", ["u8", "f32"])
def test_counts_and_means_against_float64(dev, be, real, name):
    dt = TORCH_DTYPES[name]
    x = tiles_of(real, dt)
    k, z = DEFAULT
    for basis_name in NAMES:
        basis = stain_basis(basis_name)
        conc64 = qn.concentrations64(x.numpy(), basis.numpy())
        sure, near = qn.sure_and_near(conc64, k, z)
        share = qn.near_edge_share(conc64, k)
        got = StainHistograms(*be.quantify(x.to(dev), basis.to(dev), bin_log2=k, zero_bin=z), k, z)
        counts = got.counts.cpu().numpy()
        moved = int(np.maximum(counts - sure, 0).sum())
        mean64 = conc64.reshape(6, 3, -1).mean(axis=-1)
        err = float(np.abs(got.mean().cpu().numpy() - mean64).max())
        print(f"{name} {basis_name}: near-edge share max {share.max():.4f} (cap 0.02), values outside their sure bin {moved} of {counts.sum()}, "
              f"max |mean - mean64| {err:.3e} (bound {CONC_TOL + 2.0**-17:.3e})")
        assert share.max() <= 0.02      # (the input condition tests/test_quantify_cpu.py asserts)
        assert (sure <= counts).all() and (counts <= sure + near).all(), (name, basis_name)
        assert err <= CONC_TOL + 2.0**-17, (name, basis_name, err)
        assert got.pixels.cpu().tolist() == [256 * 256] * 6


# ------------------------------------------------------------------------------------------------ 3. pooling
def test_pooling_is_exact_and_calls_repeat(dev, real):
    cd = ColorDeconvolution("hdab", device=dev)
    a, b = real[:4].to(dev), real[4:].to(dev)
    qa, qb = cd.quantify(a), cd.quantify(b)
    assert isinstance(qa, StainHistograms) and qa.counts.shape == (4, 3, 256) and qa.sums.shape == (4, 3) and qa.pixels.shape == (4,) and (qa.bin_log2, qa.zero_bin) == DEFAULT
    pa = cd.quantify(a, pooled=True)
    assert pa.counts.shape == (1, 3, 256) and pa.sums.shape == (1, 3) and pa.pixels.shape == (1,)
    assert torch.equal(pa.counts[0], qa.counts.sum(0)) and torch.equal(pa.sums[0], qa.sums.sum(0)) and int(pa.pixels[0]) == int(qa.pixels.sum())
    both = cd.quantify(torch.cat([a, b]), pooled=True)
    for pooled in (StainHistograms.pool(qa, qb), StainHistograms.pool(pa, cd.quantify(b, pooled=True))):
        assert torch.equal(pooled.counts, both.counts) and torch.equal(pooled.sums, both.sums) and torch.equal(pooled.pixels, both.pixels)
    again = cd.quantify(a)
    assert torch.equal(again.counts, qa.counts) and torch.equal(again.sums, qa.sums) and torch.equal(again.pixels, qa.pixels)
    again = cd.quantify(torch.cat([a, b]), pooled=True)      # (pooled: every workgroup adds into the same row)
    assert torch.equal(again.counts, both.counts) and torch.equal(again.sums, both.sums) and torch.equal(again.pixels, both.pixels)
    single = cd.quantify(real[0].to(dev))      # CHW
    assert single.counts.shape == (1, 3, 256) and torch.equal(single.counts[0], qa.counts[0]) and torch.equal(single.sums[0], qa.sums[0])
    last = ColorDeconvolution("hdab", device=dev, channel_axis=-1).quantify(nhwc(real[:4]).to(dev))
    assert torch.equal(last.counts, qa.counts) and torch.equal(last.sums, qa.sums) and torch.equal(last.pixels, qa.pixels)
    empty = cd.quantify(real[:0].to(dev))
    assert empty.counts.shape == (0, 3, 256) and empty.pixels.shape == (0,)
    none = cd.quantify(real[:0].to(dev), pooled=True)
    assert none.counts.shape == (1, 3, 256) and int(none.counts.sum()) == 0 and int(none.pixels.sum()) == 0


# ------------------------------------------------------------------------------------------------ 4. masks
@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f64"])
def test_masks(dev, be, lib, real, per_tile, name):
    dt = TORCH_DTYPES[name]
    rng = np.random.default_rng(5)
    for what, tiles8 in (("real", real[:3]), ("160x112", real[:3, :, :160, :112].contiguous()), ("67x65", real[:3, :, 11:78, 5:70].contiguous())):
        x = tiles_of(tiles8, dt).to(dev)
        n, _, h, w = x.shape
        keep = rng.random((n, h, w)) < 0.4
        keep[1] = False      # an all-zero mask for one tile
        mask = torch.from_numpy(keep.astype(np.uint8) * 3).to(dev)      # (non-zero = in)
        for basis in (stain_basis("hdab").to(dev), per_tile[:n].contiguous()):
            conc = separated(be, x, basis)
            want = qn.histogram_of(conc, *DEFAULT, keep=keep)
            got = be.quantify(x, basis, masking=(mask, 0.8))
            same(got, want, (what, name, "explicit"))
            assert got[2].cpu().tolist() == keep.reshape(n, -1).sum(axis=1).tolist() and int(got[0][1].sum()) == 0 and int(got[1][1].abs().sum()) == 0
            same(be.quantify(x, basis, masking=(mask.bool(), 0.8), per_tile=False), qn.pooled(*want), (what, name, "bool mask, pooled"))
            same(raw_quantify(lib, x, basis, *DEFAULT, mask=unaligned_copy(mask)), want, (what, name, "misaligned mask: the scalar path"))
            same(raw_quantify(lib, unaligned_copy(x), basis, *DEFAULT, mask=mask), want, (what, name, "misaligned pixels"))
            same(be.quantify(x, basis, masking=(torch.zeros_like(mask), 0.8)), tuple(np.zeros_like(t) for t in want), (what, name, "all-zero mask"))
        # the rule: the explicit call with tissue_mask()'s bytes
        basis = stain_basis("hdab")
        rule = ColorDeconvolution(basis, device=dev, mask="luminosity").quantify(x)
        bytes_, tissue = tissue_mask(x)
        explicit = ColorDeconvolution(basis, device=dev).quantify(x, mask=bytes_)
        assert torch.equal(rule.counts, explicit.counts) and torch.equal(rule.sums, explicit.sums) and torch.equal(rule.pixels, explicit.pixels)
        assert torch.equal(rule.pixels, tissue)
        by_call = ColorDeconvolution(basis, device=dev).quantify(x, mask="luminosity")
        assert torch.equal(by_call.counts, rule.counts)
        # a basis row with a NaN: a zero row for that tile only, masked or not
        broken = per_tile[:n].clone()
        broken[2, 1, 1] = float("nan")
        clean = be.quantify(x, per_tile[:n].contiguous())
        for masking in (None, (torch.ones_like(mask), 0.8)):
            got = be.quantify(x, broken, masking=masking)
            assert int(got[0][2].sum()) == 0 and int(got[1][2].abs().sum()) == 0 and int(got[2][2]) == 0, (what, name)
            assert torch.equal(got[0][:2], clean[0][:2]) and torch.equal(got[1][:2], clean[1][:2]) and torch.equal(got[2][:2], clean[2][:2]), (what, name)


# ------------------------------------------------------------------------------------------------ 5. non-finite pixels
@pytest.mark.parametrize("shape", ["160x112", "67x65"])
def test_non_finite_pixels_are_not_counted(dev, be, real, shape):
    h, w = (160, 112) if shape == "160x112" else (67, 65)
    clean = tiles_of(real[:2, :, 11 : 11 + h, 5 : 5 + w].contiguous(), torch.float32)
    x = clean.clone()
    bad = np.zeros((2, h, w), dtype=bool)
    rng = np.random.default_rng(11)
    values = (float("nan"), float("inf"), -0.004, -0.5)      # (255 x + 1 <= 0: no logarithm)
    for i in range(2):
        for j, (r, c) in enumerate(zip(rng.integers(0, h, 12), rng.integers(0, w, 12))):
            x[i, j % 3, r, c] = values[j % 4]
            bad[i, r, c] = True
    basis = stain_basis("hdab").to(dev)
    for last in (False, True):
        got = be.quantify(nhwc(x).to(dev) if last else x.to(dev), basis, channels_last=last)
        same(got, qn.histogram_of(separated(be, x.to(dev), basis), *DEFAULT), (shape, last, "the separation's own non-finite values"))
        same(got, qn.histogram_of(separated(be, clean.to(dev), basis), *DEFAULT, keep=~bad), (shape, last, "the rest is unchanged"))
        assert got[2].cpu().tolist() == [h * w - int(bad[i].sum()) for i in range(2)]
    mask = torch.ones((2, h, w), dtype=torch.uint8, device=dev)
    same(be.quantify(x.to(dev), basis, masking=(mask, 0.8)), qn.histogram_of(separated(be, clean.to(dev), basis), *DEFAULT, keep=~bad), (shape, "masked"))


# ------------------------------------------------------------------------------------------------ 6. the figures on device results
def test_figures_on_device_results(dev, be, real):
    cd = ColorDeconvolution("hdab", device=dev)
    x = real[:3].to(dev)
    q = cd.quantify(x)
    conc = cd.separate(x, stains=False, concentrations=True).concentrations.cpu().numpy()
    assert q.counts.device.type == "cuda" and q.mean().device.type == "cuda" and q.edges().device.type == "cuda"
    for s, (t, trio) in enumerate(((0.25, (0.125, 0.5, 1.0)), (0.15625, (0.125, 0.25, 0.5)), (0.03125, (0.03125, 0.0625, 0.125)))):
        frac, score = q.positive_fraction(s, t).cpu(), q.h_score(s, trio).cpu()
        for i in range(3):
            v = conc[i, s].ravel()
            assert float(frac[i]) == qn.positive_fraction(v, t), (s, i)
            assert abs(float(score[i]) - qn.h_score(v, trio)) <= 1e-12, (s, i)
            for p in (0.01, 0.5, 0.99, 1.0):
                assert float(q.quantile(s, p)[i]) == qn.quantile_edge(v, p, *DEFAULT), (s, i, p)
        print(f"stain {s}: positive fraction at {t}: {frac.tolist()}, H-score {score.tolist()}, median bin {q.quantile(s, 0.5).tolist()}")
    want_mean = qn.terms_of(conc).reshape(3, 3, -1).sum(-1) / 65536.0 / (256 * 256)
    np.testing.assert_allclose(q.mean().cpu().numpy(), want_mean, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ 7. capture
def test_a_captured_call_reads_new_pixels_at_replay(dev, be, lib, real):
    first, second = tiles_of(real[:2, :, :160, :112].contiguous(), torch.float32).to(dev), tiles_of(real[2:4, :, :160, :112].contiguous(), torch.float32).to(dev)
    basis = stain_basis("hed").to(dev)
    x, out = first.clone(), poisoned_rows(2, dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: the memset and one launch on one stream
        assert lib.sx_deconv_quantify(x.data_ptr(), f32, 2, 160, 112, basis.data_ptr(), 1, 5, 64, 1, out.data_ptr(), 0, _native.stream_ptr(dev)) == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    want_first = torch.cat([t.reshape(2, -1) for t in be.quantify(first, basis)], dim=1)
    assert torch.equal(out, want_first)
    x.copy_(second)
    graph.replay()
    torch.cuda.synchronize(dev)
    want_second = torch.cat([t.reshape(2, -1) for t in be.quantify(second, basis)], dim=1)
    assert torch.equal(out, want_second) and not torch.equal(want_second, want_first)
