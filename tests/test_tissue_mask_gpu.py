"""Tissue masks for Reinhard and histogram matching on the GPU: the rule against the oracle, masked statistics and outputs against the numpy
restatement of tests/_masked_numpy.py GIVEN the GPU's own mask (so that pixels on the threshold play no part), the identities between the
entry points bit for bit, degenerate tiles, and the plumbing (workspace etiquette, captured graph, nn.Module wrapper, masked reference).
Bounds: those tests/test_per_tile_gpu.py holds the unmasked per-tile paths to."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import HistogramMatching, Reinhard, StainNormalizerTransform, _native, synth, tissue_mask
from tests import _masked_numpy as mn
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu

THRESHOLD = 0.8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def small_cases():
    """uint8 batches with background: (a) stripes, (b) noise, (c) real crops, and odd sizes (no whole packs)."""
    yield "stripes", mn.striped_tiles()
    yield "noise_5x200x328", mn.noise_tiles()
    yield "real_256", mn.real_crops(256)
    for shape in [(3, 30, 30), (2, 33, 47), (1, 5, 4)]:
        yield f"odd_{shape}", synth.noise_u8((shape[0], 3, shape[1], shape[2]), 143)


def unaligned_copy(x: torch.Tensor) -> torch.Tensor:
    """The same values, dense, one element behind an aligned address."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0 or x.element_size() == 16)
    return view


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns (a NaN row of statistics equals itself)."""
    views = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
    return t.view(views[t.dtype]) if t.dtype in views else t


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_reinhard_close(got: torch.Tensor, want: torch.Tensor, what) -> None:
    diff = (got.double() - want.double()).abs()
    worst, share = diff.max().item(), (diff > 0).float().mean().item()
    print(f"masked reinhard {what} {got.dtype}: max |diff| {worst:.3e}, share differing {share:.3e}")
    if got.dtype == torch.float32:
        assert worst <= 1e-4, (what, worst)
    elif got.dtype == torch.uint8:
        assert worst <= 1 and share < 5e-3, (what, worst, share)
    else:
        assert worst <= 2.0 ** -8 and share < 2e-2, (what, worst, share)


def background_of(mask: torch.Tensor, like: torch.Tensor, last: bool = False) -> torch.Tensor:
    """The mask's background as a boolean tensor of the images' shape."""
    bg = mask == 0
    return (bg.unsqueeze(-1) if last else bg.unsqueeze(1)).expand_as(like)


def assert_background_kept(out: torch.Tensor, x: torch.Tensor, mask: torch.Tensor, what, last: bool = False) -> None:
    bg = background_of(mask, x, last)
    assert torch.equal(bits(out)[bg], bits(x)[bg]), what


# ------------------------------------------------------------------ 1. the rule against the oracle
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_rule_against_the_oracle(dev, name):
    dt = TORCH_DTYPES[name]
    cases = list(small_cases()) + [("real_1024", mn.real_images()[0]), ("real_512_test_5", mn.real_crops(512)[5:6])]
    for what, tiles in cases:
        src = synth.as_dtype(tiles, dt)
        want, decided = mn.rule_mask(mn.oracle_input(src), THRESHOLD)
        left_out = 1.0 - decided.mean()
        for layout in ("nchw", "nhwc", "unaligned"):
            x = src.to(dev)
            if layout == "nhwc":
                x = x.permute(0, 2, 3, 1).contiguous()
            elif layout == "unaligned":
                x = unaligned_copy(x)
            mask, counts = tissue_mask(x, THRESHOLD, channel_axis=-1 if layout == "nhwc" else 1)
            assert mask.dtype == torch.uint8 and mask.shape == want.shape and mask.device.type == "cuda"
            assert counts.dtype == torch.int64 and counts.shape == (src.shape[0],)
            got = mask.cpu().numpy()
            assert set(np.unique(got)) <= {0, 1}
            wrong = int(((got != 0) != want)[decided].sum())
            print(f"rule {what} {name} {layout}: tissue share {got.mean():.4f}, undecided by the oracle {left_out:.2e}, wrong among the decided {wrong}")
            assert wrong == 0, (what, name, layout, wrong)
            assert left_out <= mn.BORDER_CAP, (what, left_out)
            assert torch.equal(counts.cpu(), mask.sum(dim=(1, 2), dtype=torch.int64).cpu()), (what, layout)
    # another threshold moves the cut; counts alone / mask alone through the C ABI
    x = mn.striped_tiles().to(dev)
    lower, _ = tissue_mask(x, 0.5)
    want, decided = mn.rule_mask(x.cpu().numpy(), 0.5)
    assert not ((lower.cpu().numpy() != 0) != want)[decided].any() and lower.sum().item() < tissue_mask(x, 0.8)[0].sum().item()
    lib = _native.require()
    n, _, h, w = x.shape
    mask, counts = tissue_mask(x, THRESHOLD)
    only_mask = torch.empty_like(mask)
    only_counts = torch.full_like(counts, -1)
    u8 = _native.DTYPE_CODES[torch.uint8]
    assert lib.sx_tissue_mask(x.data_ptr(), u8, n, h, w, 0, THRESHOLD, only_mask.data_ptr(), None, _native.stream_ptr(dev)) == 0
    assert lib.sx_tissue_mask(x.data_ptr(), u8, n, h, w, 0, THRESHOLD, None, only_counts.data_ptr(), _native.stream_ptr(dev)) == 0
    assert torch.equal(only_mask, mask) and torch.equal(only_counts, counts)


# ------------------------------------------------------------------ 2. statistics, 3. outputs: Reinhard
@pytest.mark.parametrize("name", ["f32", "u8", "bf16"])
def test_reinhard_masked_vs_restatement(dev, name):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    dt = TORCH_DTYPES[name]
    be = ReinhardHIP(dev)
    ref_mean, ref_std = so.reinhard_fit(synth.reference_tile(96, 96).numpy())
    rm, rs = torch.from_numpy(ref_mean), torch.from_numpy(ref_std)
    for what, tiles in small_cases():
        src = synth.as_dtype(tiles, dt)
        x = src.to(dev)
        mask, counts = tissue_mask(x, THRESHOLD)
        m = mask.cpu().numpy() != 0
        xin = mn.oracle_input(src)
        for per_tile in (True, False):
            mean, std, n_tissue = be.masked_statistics(x, None, THRESHOLD, per_tile=per_tile)
            w_mean, w_std, w_n = mn.reinhard_stats(xin, m, per_tile)
            assert torch.equal(n_tissue.cpu(), torch.from_numpy(w_n)), (what, per_tile)
            np.testing.assert_allclose(mean.cpu().numpy(), w_mean, rtol=0, atol=2e-3, err_msg=f"{what} {per_tile}")      # LAB units (0..255); NaN rows equal NaN rows
            np.testing.assert_allclose(std.cpu().numpy(), w_std, rtol=1e-4, atol=1e-3, err_msg=f"{what} {per_tile}")
            if per_tile:
                assert torch.equal(n_tissue, counts)
            got, t_mean, t_std, t_n = be.transform_masked(x, rm, rs, None, THRESHOLD, per_tile=per_tile, return_statistics=True)
            assert same_bits(t_mean, mean) and same_bits(t_std, std) and torch.equal(t_n, n_tissue)      # (NaN rows: the same bits)
            want = mn.oracle_cast(mn.reinhard_transform(xin, ref_mean, ref_std, m, per_tile), dt)
            assert got.dtype == dt and got.shape == src.shape
            assert_reinhard_close(got.cpu(), want, (what, "tile" if per_tile else "batch"))
            assert_background_kept(got, x, mask, what)
            if what == "noise_5x200x328":      # the fallback with single elements: an unaligned view, rule and explicit mask
                # (it adds the pixels up in another order than the pack path: the oracle's bounds, as for the unmasked call -- not the pack path's bits)
                xu = unaligned_copy(x)
                got_u = be.transform_masked(xu, rm, rs, None, THRESHOLD, per_tile=per_tile)
                assert_reinhard_close(got_u.cpu(), want, (what, "unaligned", "tile" if per_tile else "batch"))
                assert_background_kept(got_u, x, mask, what)
                assert same_bits(be.transform_masked(xu, rm, rs, unaligned_copy(mask), THRESHOLD, per_tile=per_tile), got_u)


def test_reinhard_masked_real_512_in_full(dev):
    ref8 = mn.real_crops(512)[:1]
    for dt in (torch.uint8, torch.float32, torch.bfloat16):
        src = synth.as_dtype(mn.real_crops(512), dt)
        x, ref = src.to(dev), synth.as_dtype(ref8, dt).to(dev)
        norm = Reinhard(device=dev, backend="torch_hip", statistics="tile", mask="luminosity", luminosity_threshold=THRESHOLD).fit(ref)
        mask, _ = tissue_mask(x, THRESHOLD)
        ref_mask, _ = tissue_mask(ref, THRESHOLD)
        w_mean, w_std = mn.reinhard_fit(mn.oracle_input(synth.as_dtype(ref8, dt)), ref_mask.cpu().numpy() != 0)
        np.testing.assert_allclose(norm._reference_mean.cpu().numpy(), w_mean, rtol=0, atol=2e-3)      # `fit` with a masked reference
        np.testing.assert_allclose(norm._reference_std.cpu().numpy(), w_std, rtol=1e-4, atol=1e-3)
        got = norm.transform(x)
        want = mn.oracle_cast(mn.reinhard_transform(mn.oracle_input(src), norm._reference_mean.cpu().numpy(), norm._reference_std.cpu().numpy(), mask.cpu().numpy() != 0, True), dt)
        assert_reinhard_close(got.cpu(), want, "real 6x3x512x512 (tissue share 0.10 in the last tile)")
        assert_background_kept(got, x, mask, dt)
        glass = x[5].float()[background_of(mask, x)[5]]
        assert glass.numel() > 0.8 * x[5].numel()      # test_5: the tile that is mostly glass comes back with its glass untouched


# ------------------------------------------------------------------ 2. statistics, 3. outputs: histogram matching
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_hm_masked_bit_exact(dev, name, layout):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP

    dt = TORCH_DTYPES[name]
    axis = 1 if layout == "nchw" else -1
    last = axis == -1
    be = HistogramMatchingHIP(dev, channel_axis=axis)
    ref8 = synth.reference_tile(96, 96)
    cases = list(small_cases()) + [("real_1024", mn.real_images()[0][:2])]
    for what, tiles in cases:
        src, ref = synth.as_dtype(tiles, dt), synth.as_dtype(ref8, dt)
        if last:
            src, ref = src.permute(0, 2, 3, 1).contiguous(), ref.permute(0, 2, 3, 1).contiguous()
        hists = so.hm_fit(mn.oracle_input(ref), channel_axis=axis)
        ref_dev = [torch.from_numpy(hh).to(dev) for hh in hists]
        x = src.to(dev)
        mask, counts = tissue_mask(x, THRESHOLD, channel_axis=axis)
        m = mask.cpu().numpy() != 0
        for per_tile in (True, False):
            got, tab = be.transform_masked(x, ref_dev, None, THRESHOLD, per_tile=per_tile, return_tables=True)
            want, w_tab = mn.hm_transform(mn.oracle_input(src), hists, m, per_tile, axis, return_tables=True)
            np.testing.assert_array_equal(tab["counts"].cpu().numpy(), w_tab["counts"], err_msg=f"{what} counts")
            np.testing.assert_array_equal(tab["tissue"].cpu().numpy(), w_tab["tissue"], err_msg=f"{what} tissue")
            live = w_tab["tissue"] > 0      # (a set without tissue has no LUT worth the name: nothing reads it)
            np.testing.assert_array_equal(tab["lut"].cpu().numpy()[live], w_tab["lut"][live], err_msg=f"{what} lut")
            assert got.dtype == dt and got.shape == src.shape
            assert same_bits(got.cpu(), mn.oracle_cast(want, dt)), (what, name, layout, per_tile)
            assert_background_kept(got, x, mask, what, last)
            assert same_bits(be.transform_masked(x, ref_dev, mask, THRESHOLD, per_tile=per_tile), got), (what, "explicit mask")
            assert be.workspace_status() == 0
            if what == "noise_5x200x328":      # the fallback with single elements
                xu = unaligned_copy(x)
                assert same_bits(be.transform_masked(xu, ref_dev, None, THRESHOLD, per_tile=per_tile), got)
                assert same_bits(be.transform_masked(xu, ref_dev, unaligned_copy(mask), THRESHOLD, per_tile=per_tile), got)
        # fit on a masked reference: the normalised tissue histograms
        got_hists = be.compute_reference_histograms_masked(x, None, THRESHOLD)
        for c, w_hist in enumerate(mn.hm_fit(mn.oracle_input(src), m, axis)):
            np.testing.assert_array_equal(got_hists[c].cpu().numpy(), w_hist, err_msg=f"{what} fit")
        assert int(be.last_tissue_count.item()) == int(m.sum()) and be.workspace_status() == 0
        for c, hh in enumerate(be.compute_reference_histograms_masked(x, mask, THRESHOLD)):
            assert torch.equal(hh, got_hists[c])


# ------------------------------------------------------------------ 4. identities, all bit for bit
def test_identities(dev):
    from stainx_amd import ColorStatistics
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP

    rb = ReinhardHIP(dev)
    ref = synth.reference_tile(96, 96).to(dev)
    rm, rs = rb.compute_reference_mean_std(ref)
    batches = [("u8", mn.noise_tiles()), ("f32", synth.as_dtype(mn.noise_tiles(), torch.float32)), ("bf16", synth.as_dtype(mn.striped_tiles(), torch.bfloat16)),
               ("stripes", mn.striped_tiles()), ("odd", synth.as_dtype(synth.noise_u8((2, 3, 33, 47), 9), torch.float32)),
               ("grey_64x256", synth.as_dtype(synth.noise_u8((64, 3, 256, 256), 31), torch.float32))]      # (large enough for the unmasked call's 8-bit codes)
    for what, x in batches:
        x = x.to(dev)
        n = x.shape[0]
        mask, counts = tissue_mask(x, THRESHOLD)
        ones = torch.ones_like(mask)
        for per_tile in (True, False):
            # rule == explicit mask made by tissue_mask (statistics and outputs)
            got, mean, std, cnt = rb.transform_masked(x, rm, rs, None, THRESHOLD, per_tile=per_tile, return_statistics=True)
            e_got, e_mean, e_std, e_cnt = rb.transform_masked(x, rm, rs, mask, THRESHOLD, per_tile=per_tile, return_statistics=True)
            assert same_bits(e_got, got) and same_bits(e_mean, mean) and same_bits(e_std, std) and torch.equal(e_cnt, cnt), (what, per_tile)
            assert same_bits(rb.transform_masked(x, rm, rs, mask.bool().unsqueeze(1), THRESHOLD, per_tile=per_tile), got)      # (N, 1, H, W) bool
            s_mean, s_std, s_cnt = rb.masked_statistics(x, None, THRESHOLD, per_tile=per_tile)
            assert same_bits(s_mean, mean) and same_bits(s_std, std) and torch.equal(s_cnt, cnt)
            # transform == apply(estimate)
            assert same_bits(rb.apply_statistics_masked(x, mean, std, rm, rs, None, THRESHOLD), got), (what, per_tile)
            assert same_bits(rb.apply_statistics_masked(x, mean, std, rm, rs, mask, THRESHOLD), got), (what, per_tile)
            # all-ones explicit mask == the unmasked call of the same entry point
            o_got, o_mean, o_std, o_cnt = rb.transform_masked(x, rm, rs, ones, THRESHOLD, per_tile=per_tile, return_statistics=True)
            if per_tile:
                u_got, u_mean, u_std = rb.transform_tiles(x, rm, rs, return_statistics=True)
            else:
                u_got = rb.transform(x, rm, rs)
                u_mean, u_std = (t.reshape(1, 3) for t in rb.compute_reference_mean_std(x))
            assert same_bits(o_mean, u_mean) and same_bits(o_std, u_std), (what, per_tile)
            assert same_bits(o_got, u_got), (what, per_tile)
            assert int(o_cnt.sum().item()) == x.numel() // 3
            assert same_bits(rb.apply_statistics_masked(x, u_mean, u_std, rm, rs, ones, THRESHOLD), rb.apply_statistics(x, u_mean, u_std, rm, rs))
        # the classes: rule on the normaliser, explicit mask on a normaliser built without
        for statistics in ("tile", "batch"):
            masked = Reinhard(device=dev, backend="torch_hip", statistics=statistics, mask="luminosity", luminosity_threshold=THRESHOLD).fit(ref)
            plain = Reinhard(device=dev, backend="torch_hip", statistics=statistics).fit(ref, mask=tissue_mask(ref, THRESHOLD)[0])
            assert same_bits(masked._reference_mean, plain._reference_mean) and same_bits(masked._reference_std, plain._reference_std)
            got = masked.transform(x)
            assert same_bits(plain.transform(x, mask=mask), got) and same_bits(plain.transform(x, mask="luminosity"), got), (what, statistics)
            est = masked.estimate(x, pooled=statistics == "batch")
            assert isinstance(est, ColorStatistics) and est.mean.shape == ((n, 3) if statistics == "tile" else (1, 3)) and est.std.dtype == torch.float32
            assert same_bits(masked.apply(x, est), got) and same_bits(plain.apply(x, est, mask=mask), got), (what, statistics)
            assert same_bits(plain.estimate(x, pooled=statistics == "batch", mask=mask).mean, est.mean)
            assert same_bits(masked.fit_transform(ref), masked.transform(ref))
            unmasked = Reinhard(device=dev, backend="torch_hip", statistics=statistics).fit(ref)
            assert same_bits(unmasked.transform(x, mask=ones), unmasked.transform(x)), (what, statistics)
    # histogram matching: all-ones == unmasked (per tile and pooled, both layouts); rule == explicit is asserted in test_hm_masked_bit_exact
    for axis in (1, -1):
        hb = HistogramMatchingHIP(dev, channel_axis=axis)
        for what, x in batches[:5]:
            x = x.to(dev)
            r = ref
            if axis == -1:
                x, r = x.permute(0, 2, 3, 1).contiguous(), ref.permute(0, 2, 3, 1).contiguous()
            hists = hb.compute_reference_histograms(r)
            ones = torch.ones(x.shape[:3] if axis == -1 else (x.shape[0], x.shape[2], x.shape[3]), dtype=torch.uint8, device=dev)
            assert same_bits(hb.transform_masked(x, hists, ones, THRESHOLD, per_tile=True), hb.transform_tiles(x, hists)), (what, axis)
            assert same_bits(hb.transform_masked(x, hists, ones, THRESHOLD, per_tile=False), hb.transform(x, hists)), (what, axis)
            ones_r = torch.ones(r.shape[:3] if axis == -1 else (1, r.shape[2], r.shape[3]), dtype=torch.bool, device=dev)
            for a, b in zip(hb.compute_reference_histograms_masked(r, ones_r, THRESHOLD), hists):
                assert torch.equal(a, b)
            for statistics in ("tile", "batch"):
                masked = HistogramMatching(device=dev, backend="torch_hip", statistics=statistics, channel_axis=axis, mask="luminosity").fit(r)
                plain = HistogramMatching(device=dev, backend="torch_hip", statistics=statistics, channel_axis=axis).fit(r, mask=tissue_mask(r, THRESHOLD, channel_axis=axis)[0])
                got = masked.transform(x)
                assert same_bits(plain.transform(x, mask=tissue_mask(x, THRESHOLD, channel_axis=axis)[0]), got), (what, axis, statistics)
                assert same_bits(masked.fit_transform(r), masked.transform(r))


def test_tiles_do_not_depend_on_their_neighbours(dev):
    x = torch.cat([mn.striped_tiles()[1:4], mn.noise_tiles((2, 3, 96, 96), 11)])
    y = x.clone()
    y[2] = synth.background_stripes(synth.noise_u8((3, 3, 96, 96), 13))[1]
    ref = synth.reference_tile(96, 96).to(dev)
    keep = [0, 1, 3, 4]
    for cls in (Reinhard, HistogramMatching):
        tile = cls(device=dev, backend="torch_hip", statistics="tile", mask="luminosity").fit(ref)
        a, b = tile.transform(x.to(dev)).cpu(), tile.transform(y.to(dev)).cpu()
        assert torch.equal(a[keep], b[keep]), cls.__name__      # replacing tile 2 changes tile 2 only
        assert not torch.equal(a[2], b[2])
        if cls is HistogramMatching:      # a tile alone, in another order: the same bits (Reinhard's reduction order follows the grid)
            assert torch.equal(tile.transform(x[3:4].to(dev)).cpu(), a[3:4])
            assert torch.equal(tile.transform(x.flip(0).contiguous().to(dev)).cpu().flip(0), a)
        pooled = cls(device=dev, backend="torch_hip", mask="luminosity").fit(ref)
        pa, pb = pooled.transform(x.to(dev)).cpu(), pooled.transform(y.to(dev)).cpu()
        for i in keep:      # the pooled mode is batch-coupled: every other tile moves
            assert (pa[i].int() - pb[i].int()).abs().max().item() >= 1, (cls.__name__, i)


# ------------------------------------------------------------------ 5. degenerate tiles
def test_degenerate_tiles(dev):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP

    rb, hb = ReinhardHIP(dev), HistogramMatchingHIP(dev)
    ref = synth.reference_tile(96, 96).to(dev)
    rm, rs = rb.compute_reference_mean_std(ref)
    hists = hb.compute_reference_histograms(ref)
    for dt in (torch.uint8, torch.float32, torch.bfloat16):
        x = synth.as_dtype(mn.striped_tiles(), dt).to(dev)      # tile 5: all background under the rule
        mask, counts = tissue_mask(x, THRESHOLD)
        assert counts[5].item() == 0 and counts[0].item() == 96 * 96
        one = mask.clone()
        one[2] = 0
        one[2, 40, 50] = 1      # exactly one tissue pixel in tile 2
        none = mask.clone()
        none[3] = 0             # an all-zero explicit mask for tile 3
        base_r = rb.transform_masked(x, rm, rs, None, THRESHOLD, per_tile=True)
        base_h = hb.transform_masked(x, hists, None, THRESHOLD, per_tile=True)
        assert same_bits(base_r[5], x[5]) and same_bits(base_h[5], x[5]), dt
        mean, std, n_tissue = rb.masked_statistics(x, None, THRESHOLD, per_tile=True)
        assert bool(torch.isnan(mean[5]).all()) and bool(torch.isnan(std[5]).all()) and bool(torch.isfinite(mean[:5]).all()) and bool(torch.isfinite(std[:5]).all())
        for explicit, tile, count in ((one, 2, 1), (none, 3, 0)):
            got_r, mean, std, n_tissue = rb.transform_masked(x, rm, rs, explicit, THRESHOLD, per_tile=True, return_statistics=True)
            got_h, tab = hb.transform_masked(x, hists, explicit, THRESHOLD, per_tile=True, return_tables=True)
            assert n_tissue[tile].item() == count and tab["tissue"][tile].item() == count
            assert bool(torch.isnan(mean[tile]).all()) and bool(torch.isnan(std[tile]).all())      # fewer than two tissue pixels: no statistics
            assert same_bits(got_r[tile], x[tile]), (dt, tile)      # Reinhard: the tile passes through
            others = [i for i in range(6) if i != tile]
            assert same_bits(got_r[others], base_r[others]) and same_bits(got_h[others], base_h[others]), (dt, tile)
            if count == 0:
                assert same_bits(got_h[tile], x[tile])
            else:      # histogram matching: one tissue pixel is matched (hm_lut with n = 1), everything else is the input's
                bg = background_of(explicit, x)[tile]
                assert torch.equal(bits(got_h[tile])[bg], bits(x[tile])[bg])
            est = Reinhard(device=dev, backend="torch_hip", statistics="tile").fit(ref).estimate(x, mask=explicit)
            assert bool(torch.isnan(est.mean[tile]).all()) and bool(torch.isnan(est.std[tile]).all())
        # pooled batch without tissue: everything passes through
        glass = x[5:6].repeat(3, 1, 1, 1).contiguous()
        assert same_bits(rb.transform_masked(glass, rm, rs, None, THRESHOLD, per_tile=False), glass)
        assert same_bits(hb.transform_masked(glass, hists, None, THRESHOLD, per_tile=False), glass)
        p_mean, p_std, p_n = rb.masked_statistics(glass, None, THRESHOLD, per_tile=False)
        assert p_n.item() == 0 and bool(torch.isnan(p_mean).all()) and bool(torch.isnan(p_std).all())
        # a NaN row handed to apply: that tile is copied, the others are not touched by it
        mean, std, _ = rb.masked_statistics(x, None, THRESHOLD, per_tile=True)
        broken = std.clone()
        broken[1] = float("nan")
        got = rb.apply_statistics_masked(x, mean, broken, rm, rs, None, THRESHOLD)
        assert same_bits(got[1], x[1]) and same_bits(got[[0, 2, 3, 4, 5]], base_r[[0, 2, 3, 4, 5]])


# ------------------------------------------------------------------ 6. plumbing
def test_reinhard_masked_workspace_etiquette(dev):
    lib = _native.require()
    src = synth.as_dtype(mn.noise_tiles(), torch.float32).to(dev)
    mean = torch.tensor([150.0, 130.0, 120.0], device=dev)
    std = torch.tensor([40.0, 9.0, 12.0], device=dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    stream = _native.stream_ptr(dev)
    shapes = [src, src[:2, :, :64, :96].contiguous(), src[:5, :, :200, :200].contiguous(), src[:1].contiguous()]
    size = max(max(int(lib.sx_reinhard_masked_workspace_bytes(f32, x.shape[0], x.shape[2], x.shape[3])), int(lib.sx_reinhard_tiles_workspace_bytes(f32, x.shape[0], x.shape[2], x.shape[3])))
               for x in shapes)
    off = int(lib.sx_reinhard_workspace_status_offset())

    def status(ws):
        return int(ws[off:off + 4].view(torch.int32).item())

    def masked(x, ws, per_tile):
        out = torch.empty_like(x)
        assert lib.sx_reinhard_transform_masked(x.data_ptr(), out.data_ptr(), f32, x.shape[0], x.shape[2], x.shape[3], mean.data_ptr(), std.data_ptr(), None, THRESHOLD, per_tile,
                                                None, None, None, ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def tiles(x, ws):
        out = torch.empty_like(x)
        assert lib.sx_reinhard_transform_tiles(x.data_ptr(), out.data_ptr(), f32, x.shape[0], x.shape[2], x.shape[3], mean.data_ptr(), std.data_ptr(), None, None,
                                               ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def ready(x, ws):
        out = torch.empty_like(x)
        assert lib.sx_reinhard_transform_ready(x.data_ptr(), out.data_ptr(), f32, x.shape[0], x.shape[2], x.shape[3], mean.data_ptr(), std.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        return out

    clean = torch.zeros(size, dtype=torch.uint8, device=dev)
    want = {(k, p): masked(x, clean, p) for k, x in enumerate(shapes) for p in (0, 1)}
    want_tiles = [tiles(x, clean) for x in shapes]
    want_ready = [ready(x, clean) for x in shapes]
    m = tissue_mask(src, THRESHOLD)[0].cpu().numpy() != 0
    oracle = torch.from_numpy(mn.reinhard_transform(src.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy(), m, True))
    assert (want[(0, 1)].cpu() - oracle).abs().max().item() <= 1e-4
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
    assert torch.equal(masked(src, ws, 1), want[(0, 1)]) and status(ws) == 0            # garbage in: the call clears what it needs ...
    assert torch.equal(ready(src, ws), want_ready[0]) and status(ws) == 0               # ... and leaves the workspace ready
    ws.fill_(0xA5)
    assert torch.equal(masked(src, ws, 0), want[(0, 0)]) and status(ws) == 0
    assert torch.equal(ready(src, ws), want_ready[0]) and status(ws) == 0
    for _ in range(2):
        order = list(range(len(shapes))) + list(range(len(shapes)))[::-1]
        for k in order:
            for per_tile in (1, 0):
                assert torch.equal(masked(shapes[k], ws, per_tile), want[(k, per_tile)]) and status(ws) == 0, (tuple(shapes[k].shape), per_tile)
                assert torch.equal(ready(shapes[k - 1], ws), want_ready[k - 1]) and status(ws) == 0, tuple(shapes[k - 1].shape)
            assert torch.equal(tiles(shapes[k - 2], ws), want_tiles[k - 2]) and status(ws) == 0


def test_hm_masked_workspace_etiquette(dev):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP

    lib = _native.require()
    be = HistogramMatchingHIP(dev)
    src = mn.noise_tiles((3, 3, 200, 328), 7).to(dev)
    ref = torch.stack(be.compute_reference_histograms(synth.noise_u8((1, 3, 200, 328), 8).to(dev))).contiguous()
    hists = [r.cpu().numpy() for r in ref]
    u8 = _native.DTYPE_CODES[torch.uint8]
    stream = _native.stream_ptr(dev)
    shapes = [src, src[:2, :, :64, :96].contiguous(), src[:1].contiguous()]

    def rule(x):
        return tissue_mask(x, THRESHOLD)[0].cpu().numpy() != 0

    want_masked = {(k, p): torch.from_numpy(mn.hm_transform(x.cpu().numpy(), hists, rule(x), bool(p))).to(dev) for k, x in enumerate(shapes) for p in (0, 1)}
    want_tiles = [torch.from_numpy(np.concatenate([so.hm_transform(x[i:i + 1].cpu().numpy(), hists) for i in range(x.shape[0])])).to(dev) for x in shapes]
    want_pooled = [torch.from_numpy(so.hm_transform(x.cpu().numpy(), hists)).to(dev) for x in shapes]
    size = max(max(int(lib.sx_hm_masked_workspace_bytes(x.shape[0], x.shape[2], x.shape[3])), int(lib.sx_hm_tiles_workspace_bytes(x.shape[0], x.shape[2], x.shape[3]))) for x in shapes)
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
    off = int(lib.sx_hm_workspace_status_offset())

    def status():
        return int(ws[off:off + 4].view(torch.int32).item())

    def masked(x, per_tile):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_masked(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), None, THRESHOLD, per_tile, None, None, None,
                                          ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def tiles(x):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_tiles(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), None, None, ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def ready(x):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_ready(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        return out

    assert torch.equal(masked(src, 1), want_masked[(0, 1)]) and status() == 0                # garbage in
    assert torch.equal(ready(src), want_pooled[0]) and status() == 0                         # READY out
    for _ in range(2):
        for k in (0, 1, 2, 2, 1, 0):
            for per_tile in (1, 0):
                assert torch.equal(masked(shapes[k], per_tile), want_masked[(k, per_tile)]) and status() == 0, (k, per_tile)
                assert torch.equal(ready(shapes[k - 1]), want_pooled[k - 1]) and status() == 0
            assert torch.equal(tiles(shapes[k - 2]), want_tiles[k - 2]) and status() == 0


def test_apply_stats_masked_in_a_captured_graph_reads_statistics_and_mask_at_replay(dev):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    lib = _native.require()
    be = ReinhardHIP(dev)
    x = synth.as_dtype(mn.striped_tiles()[:4], torch.float32).to(dev)
    rm, rs = be.compute_reference_mean_std(synth.reference_tile(96, 96).to(dev))
    first_mask = tissue_mask(x, THRESHOLD)[0]
    first_mean, first_std, _ = be.masked_statistics(x, first_mask, THRESHOLD, per_tile=True)
    new_mask = first_mask.clone()
    new_mask[:, :48] = 0
    new_mean, new_std = first_mean * 1.02 + 1.0, first_std * 0.9
    mean, std, mask = first_mean.clone(), first_std.clone(), first_mask.clone()
    out = torch.empty_like(x)
    f32 = _native.DTYPE_CODES[torch.float32]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: one launch on one stream
        assert lib.sx_reinhard_apply_stats_masked(x.data_ptr(), out.data_ptr(), f32, 4, 96, 96, mean.data_ptr(), std.data_ptr(), 4, rm.data_ptr(), rs.data_ptr(),
                                                  mask.data_ptr(), THRESHOLD, _native.stream_ptr(dev)) == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    first = be.apply_statistics_masked(x, first_mean, first_std, rm, rs, first_mask, THRESHOLD)
    assert torch.equal(out, first)
    mean.copy_(new_mean)
    std.copy_(new_std)
    mask.copy_(new_mask)
    graph.replay()
    torch.cuda.synchronize(dev)
    want = be.apply_statistics_masked(x, new_mean, new_std, rm, rs, new_mask, THRESHOLD)
    assert torch.equal(out, want) and not torch.equal(want, first)
    assert torch.equal(out[:, :, :48], x[:, :, :48])      # the new mask's background, read at replay


def test_masked_normalisers_pass_through_the_transform_module(dev):
    x = torch.cat([mn.striped_tiles()[1:4], mn.noise_tiles((2, 3, 96, 96), 11)])
    ref = synth.reference_tile(96, 96)
    for cls in (Reinhard, HistogramMatching):
        for statistics in ("tile", "batch"):
            inner = cls(device=dev, backend="torch_hip", statistics=statistics, mask="luminosity", luminosity_threshold=THRESHOLD)
            module = StainNormalizerTransform(normalizer=inner, reference=ref.to(dev), device=dev)
            got = module(x.to(dev))
            assert torch.equal(got, inner.transform(x.to(dev)))
            mask, _ = tissue_mask(x.to(dev), THRESHOLD)
            assert_background_kept(got, x.to(dev), mask, cls.__name__)
            m = mask.cpu().numpy() != 0
            ref_m = tissue_mask(ref.to(dev), THRESHOLD)[0].cpu().numpy() != 0
            if cls is Reinhard:
                want = mn.reinhard_transform(x.numpy(), *mn.reinhard_fit(ref.numpy(), ref_m), m, statistics == "tile")
                assert (got.cpu().int() - torch.from_numpy(want).int()).abs().max().item() <= 1
            else:
                want = mn.hm_transform(x.numpy(), mn.hm_fit(ref.numpy(), ref_m), m, statistics == "tile")
                assert torch.equal(got.cpu(), torch.from_numpy(want))
            assert torch.equal(module(x[3].to(dev)), got[3]) or not (cls is HistogramMatching and statistics == "tile")      # a CHW tile alone
