"""Per-tile source statistics for Reinhard and histogram matching on the GPU, through the C ABI and through the classes.  Every expected
value comes from the CPU oracle applied tile by tile; the tolerances are the ones tests/test_siblings_gpu.py holds the pooled paths to."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import _native, synth
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def mixed_batch():
    """Three Beer-Lambert tiles and two noise tiles, uint8, with their reference; and the same batch with tile 2 replaced."""
    he = synth.he_batch(3, 96, 96, seed0=500, scale_step=0.1)
    x = torch.cat([he[:1], synth.noise_u8((1, 3, 96, 96), 11), he[1:2], synth.noise_u8((1, 3, 96, 96), 12), he[2:3]])
    y = x.clone()
    y[2] = synth.noise_u8((1, 3, 96, 96), 13)[0]
    return x, y, synth.reference_tile(96, 96)


def oracle_input(x: torch.Tensor) -> np.ndarray:
    return x.numpy() if x.dtype in (torch.uint8, torch.float32) else x.float().numpy()      # (bf16 / f16 -> float32 is exact)


def oracle_cast(arr: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dtype)      # (the reference's dtype gate: the float32 result cast by torch)


def reinhard_oracle_tiles(x: torch.Tensor, mean, std) -> torch.Tensor:
    xin = oracle_input(x)
    return oracle_cast(np.concatenate([so.reinhard_transform(xin[i:i + 1], mean, std) for i in range(x.shape[0])]), x.dtype)


def hm_oracle_tiles(x: torch.Tensor, hists, axis: int) -> torch.Tensor:
    xin = oracle_input(x)
    return oracle_cast(np.concatenate([so.hm_transform(xin[i:i + 1], hists, channel_axis=axis) for i in range(x.shape[0])]), x.dtype)


def assert_reinhard_close(got: torch.Tensor, want: torch.Tensor, what) -> None:
    diff = (got.double() - want.double()).abs()
    worst, share = diff.max().item(), (diff > 0).float().mean().item()
    print(f"reinhard per tile {what} {got.dtype}: max |diff| {worst:.3e}, share differing {share:.3e}")
    if got.dtype == torch.float32:
        assert worst <= 1e-4, (what, worst)
    elif got.dtype == torch.uint8:
        assert worst <= 1 and share < 5e-3, (what, worst, share)
    else:
        assert worst <= 2.0 ** -8 and share < 2e-2, (what, worst, share)


def unaligned_copy(x: torch.Tensor) -> torch.Tensor:
    """The same values, dense, at an address that is not 16-byte aligned (one element behind an aligned one)."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


# ------------------------------------------------------------------ independence
def test_tiles_do_not_depend_on_their_neighbours(dev):
    from stainx_amd import HistogramMatching, Reinhard

    x, y, ref = mixed_batch()
    keep = [0, 1, 3, 4]
    for cls in (Reinhard, HistogramMatching):
        tile = cls(device=dev, backend="torch_hip", statistics="tile").fit(ref.to(dev))
        a, b = tile.transform(x.to(dev)).cpu(), tile.transform(y.to(dev)).cpu()
        assert torch.equal(a[keep], b[keep]), cls.__name__
        assert not torch.equal(a[2], b[2])
        # a tile alone, in another batch size, in another order: the same bits (HM; Reinhard's reduction order follows the grid)
        if cls is HistogramMatching:
            assert torch.equal(tile.transform(x[3:4].to(dev)).cpu(), a[3:4])
            assert torch.equal(tile.transform(x.flip(0).contiguous().to(dev)).cpu().flip(0), a)
        pooled = cls(device=dev, backend="torch_hip").fit(ref.to(dev))
        pa, pb = pooled.transform(x.to(dev)).cpu(), pooled.transform(y.to(dev)).cpu()
        for i in keep:      # the pooled mode is batch-coupled, like the reference: every other tile moves
            assert (pa[i].int() - pb[i].int()).abs().max().item() > 1, (cls.__name__, i)
        assert (pa.int() - a.int()).abs().max().item() > 1


def test_independence_through_the_c_abi(dev):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP

    lib = _native.require()
    x, y, ref = mixed_batch()
    x, y = x.to(dev), y.to(dev)
    n, _, h, w = x.shape
    u8 = _native.DTYPE_CODES[torch.uint8]
    stream = _native.stream_ptr(dev)
    mean, std = ReinhardHIP(dev).compute_reference_mean_std(ref.to(dev))
    hists = torch.stack(HistogramMatchingHIP(dev).compute_reference_histograms(ref.to(dev))).contiguous()
    ws_r = torch.empty(int(lib.sx_reinhard_tiles_workspace_bytes(u8, n, h, w)), dtype=torch.uint8, device=dev)
    ws_h = torch.empty(int(lib.sx_hm_tiles_workspace_bytes(n, h, w)), dtype=torch.uint8, device=dev)
    outs = []
    for batch in (x, y):
        r, m = torch.empty_like(batch), torch.empty_like(batch)
        assert lib.sx_reinhard_transform_tiles(batch.data_ptr(), r.data_ptr(), u8, n, h, w, mean.data_ptr(), std.data_ptr(), None, None,
                                               ws_r.data_ptr(), ws_r.numel(), stream) == 0
        assert lib.sx_hm_transform_tiles(batch.data_ptr(), m.data_ptr(), u8, n, h, w, 0, hists.data_ptr(), None, None, ws_h.data_ptr(), ws_h.numel(), stream) == 0
        outs.append((r.cpu(), m.cpu()))
    for i in (0, 1, 3, 4):
        assert torch.equal(outs[0][0][i], outs[1][0][i]) and torch.equal(outs[0][1][i], outs[1][1][i]), i
    assert not torch.equal(outs[0][0][2], outs[1][0][2]) and not torch.equal(outs[0][1][2], outs[1][1][2])


# ------------------------------------------------------------------ histogram matching: bit-exact parity
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["u8", "f32", "bf16", "f16"])
def test_hm_tiles_bit_exact(dev, name, layout):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP

    dt = TORCH_DTYPES[name]
    axis = 1 if layout == "nchw" else -1
    be = HistogramMatchingHIP(dev, channel_axis=axis)
    for case, (n, h, w) in enumerate([(3, 96, 80), (4, 33, 47), (2, 1024, 1024), (3, 40, 52)]):
        src8 = torch.cat([synth.noise_u8((n - 1, 3, h, w), 43 + case), synth.he_batch(1, h, w, seed0=700 + case)])
        ref8 = synth.noise_u8((1, 3, h, w), 42)
        src, ref = synth.as_dtype(src8, dt), synth.as_dtype(ref8, dt)
        if axis == -1:
            src, ref = src.permute(0, 2, 3, 1).contiguous(), ref.permute(0, 2, 3, 1).contiguous()
        hists = so.hm_fit(oracle_input(ref), channel_axis=axis)
        ref_dev = [torch.from_numpy(hh).to(dev) for hh in hists]
        want = hm_oracle_tiles(src, hists, axis)
        x = src.to(dev)
        if case == 3:
            x = unaligned_copy(x)      # the fallback with single elements
        got = be.transform_tiles(x, ref_dev)
        assert got.dtype == dt and got.shape == src.shape
        for i in range(n):
            assert torch.equal(got[i].cpu(), want[i]), (name, layout, (n, h, w), i)
        tab = be.tile_tables()
        for i in range(n):
            tile = src[i] if axis == 1 else src[i].permute(2, 0, 1)
            levels = so.images_to_uint8(oracle_input(tile.contiguous()))[0]      # (floats: trunc(clamp(x * 255)), the reference's grey levels)
            counts = np.stack([np.bincount(levels[c].reshape(-1), minlength=256) for c in range(3)])
            np.testing.assert_array_equal(tab["counts"][i].numpy(), counts)
            assert torch.equal(be.transform(x[i:i + 1], ref_dev), got[i:i + 1]), (name, layout, (n, h, w), i)      # the pooled call on the tile alone
        assert bool((tab["lut"][:, :, 1:] >= tab["lut"][:, :, :-1]).all())


def test_hm_tiles_tables_through_the_c_abi(dev):
    lib = _native.require()
    src = torch.cat([synth.noise_u8((2, 3, 64, 80), 5), synth.he_batch(2, 64, 80, seed0=300)]).to(dev)
    hists = so.hm_fit(synth.noise_u8((1, 3, 64, 80), 6).numpy())
    ref = torch.from_numpy(np.stack(hists)).to(dev)
    n, _, h, w = src.shape
    ws = torch.full((int(lib.sx_hm_tiles_workspace_bytes(n, h, w)),), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.empty_like(src)
    counts = torch.empty((n, 3, 256), dtype=torch.int32, device=dev)
    lut = torch.empty((n, 3, 256), dtype=torch.float32, device=dev)
    assert lib.sx_hm_transform_tiles(src.data_ptr(), out.data_ptr(), _native.DTYPE_CODES[torch.uint8], n, h, w, 0, ref.data_ptr(), counts.data_ptr(),
                                     lut.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(dev)) == 0
    for i in range(n):
        want, tables = so.hm_transform(src[i:i + 1].cpu().numpy(), hists, return_tables=True)
        assert np.array_equal(out[i:i + 1].cpu().numpy(), want)
        np.testing.assert_array_equal(counts[i].cpu().numpy(), np.stack(tables["counts"]))
        np.testing.assert_array_equal(lut[i].cpu().numpy(), np.stack(tables["lut"]))


# ------------------------------------------------------------------ Reinhard: parity with the oracle, tile by tile
def reinhard_cases():
    yield "he_3x96", synth.he_batch(3, 96, 96, seed0=500, scale_step=0.1)
    yield "noise_5x200x328", synth.noise_u8((5, 3, 200, 328), 7)
    for shape in [(3, 30, 30), (2, 33, 47), (1, 17, 20), (4, 50, 50), (1, 5, 4)]:
        yield f"partial_{shape}", synth.noise_u8((shape[0], 3, shape[1], shape[2]), 143)


@pytest.mark.parametrize("name", ["f32", "u8", "bf16"])
def test_reinhard_tiles_vs_oracle(dev, name):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    dt = TORCH_DTYPES[name]
    be = ReinhardHIP(dev)
    ref_mean, ref_std = so.reinhard_fit(synth.reference_tile(96, 96).numpy())
    for what, tiles8 in reinhard_cases():
        src = synth.as_dtype(tiles8, dt)
        want = reinhard_oracle_tiles(src, ref_mean, ref_std)
        got, mean, std = be.transform_tiles(src.to(dev), torch.from_numpy(ref_mean), torch.from_numpy(ref_std), return_statistics=True)
        assert got.dtype == dt and got.shape == src.shape
        assert_reinhard_close(got.cpu(), want, what)
        stats_mean, stats_std = be.tile_statistics(src.to(dev))
        assert torch.equal(stats_mean, mean) and torch.equal(stats_std, std)
        for i in range(src.shape[0]):
            m, s = so.reinhard_fit(oracle_input(src[i:i + 1]))
            np.testing.assert_allclose(mean[i].cpu().numpy(), m, rtol=0, atol=2e-3)      # LAB units (0..255)
            np.testing.assert_allclose(std[i].cpu().numpy(), s, rtol=1e-4, atol=1e-3)
        if what == "noise_5x200x328":      # the fallback with single elements: an unaligned view
            got_u = be.transform_tiles(unaligned_copy(src.to(dev)), torch.from_numpy(ref_mean), torch.from_numpy(ref_std))
            assert_reinhard_close(got_u.cpu(), want, what + " unaligned")


@pytest.mark.parametrize("name", ["f32", "u8", "bf16"])
def test_reinhard_tiles_16x512_in_full(dev, name):
    from stainx_amd import Reinhard

    dt = TORCH_DTYPES[name]
    tiles8 = torch.cat([synth.noise_u8((8, 3, 512, 512), 21), synth.he_batch(8, 512, 512, seed0=900, scale_step=0.02)])
    src = synth.as_dtype(tiles8, dt)
    ref = synth.reference_tile(128, 128)
    norm = Reinhard(device=dev, backend="torch_hip", statistics="tile").fit(ref.to(dev))
    got = norm.transform(src.to(dev)).cpu()
    ref_mean, ref_std = so.reinhard_fit(ref.numpy())
    assert_reinhard_close(got, reinhard_oracle_tiles(src, ref_mean, ref_std), "16x3x512x512")


def test_one_pixel_tiles_have_nan_std(dev):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    mean, std = ReinhardHIP(dev).tile_statistics(synth.noise_u8((3, 3, 1, 1), 3).to(dev))
    assert bool(torch.isnan(std).all()) and bool(torch.isfinite(mean).all())      # torch.std of one value


def test_zero_variance_tile_leaves_the_others_alone(dev):
    from stainx_amd import Reinhard

    x, _, ref = mixed_batch()
    flat = x.clone()
    flat[2] = 200      # one value in every pixel: (lab - mean) / (0 + 1e-8) -- not a parity case, in the reference either
    for dt in (torch.uint8, torch.float32):
        norm = Reinhard(device=dev, backend="torch_hip", statistics="tile").fit(ref.to(dev))
        a = norm.transform(synth.as_dtype(x, dt).to(dev)).cpu()
        b = norm.transform(synth.as_dtype(flat, dt).to(dev)).cpu()      # (returns: SX_OK)
        assert torch.equal(a[[0, 1, 3, 4]], b[[0, 1, 3, 4]])


# ------------------------------------------------------------------ identities, bit for bit
def coded_batches():
    grey = synth.as_dtype(synth.noise_u8((64, 3, 256, 256), 31), torch.float32)      # float(k) / 255 in every element: the 8-bit codes apply
    mixed = grey[:20].clone()
    mixed[3] = (mixed[3] * 0.987 + 0.004)      # not grey levels
    mixed[11, 1, 17, 5] += 1e-3
    mixed = torch.cat([mixed, synth.as_dtype(synth.he_batch(4, 256, 256, seed0=40), torch.float32)])
    return (("grey", grey), ("mixed", mixed))


def test_identities(dev):
    from stainx_amd import ColorStatistics, Reinhard
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    lib = _native.require()
    be = ReinhardHIP(dev)
    stream = _native.stream_ptr(dev)
    ref = synth.reference_tile(96, 96).to(dev)
    rm, rs = be.compute_reference_mean_std(ref)
    batches = [("u8", synth.noise_u8((5, 3, 200, 328), 7)), ("f32", synth.as_dtype(synth.noise_u8((5, 3, 200, 328), 7), torch.float32)),
               ("bf16", synth.as_dtype(synth.he_batch(4, 96, 96, seed0=500, scale_step=0.1), torch.bfloat16)),
               ("odd", synth.as_dtype(synth.noise_u8((2, 3, 33, 47), 9), torch.float32)), *coded_batches()]
    for what, x in batches:
        x = x.to(dev)
        n, _, h, w = x.shape
        code = _native.DTYPE_CODES[x.dtype]
        # per tile: transform == apply(statistics); the statistics the transform reports are tile_statistics'
        got, mean, std = be.transform_tiles(x, rm, rs, return_statistics=True)
        s_mean, s_std = be.tile_statistics(x)
        assert torch.equal(mean, s_mean) and torch.equal(std, s_std), what
        assert torch.equal(be.apply_statistics(x, s_mean, s_std, rm, rs), got), what
        assert torch.equal(be.transform_tiles(x, rm, rs), got), what      # (without the outputs: the same bits)
        # pooled: apply(fit(x), one row) == the pooled transform, plain and ready, coded float32 tiles included
        p_mean, p_std = be.compute_reference_mean_std(x)
        pooled = be.transform(x, rm, rs)
        assert torch.equal(be.apply_statistics(x, p_mean, p_std, rm, rs), pooled), what
        plain = torch.empty_like(x)
        ws = torch.empty(int(lib.sx_reinhard_workspace_bytes_for(code, n, h, w)), dtype=torch.uint8, device=dev)
        assert lib.sx_reinhard_transform(x.data_ptr(), plain.data_ptr(), code, n, h, w, rm.data_ptr(), rs.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        assert torch.equal(plain, pooled), what
        out = torch.empty_like(x)
        assert lib.sx_reinhard_apply_stats(x.data_ptr(), out.data_ptr(), code, n, h, w, p_mean.data_ptr(), p_std.data_ptr(), 1, rm.data_ptr(), rs.data_ptr(), stream) == 0
        assert torch.equal(out, pooled), what
        # the classes
        tile = Reinhard(device=dev, backend="torch_hip", statistics="tile").fit(ref)
        est = tile.estimate(x)
        assert isinstance(est, ColorStatistics) and est.mean.shape == (n, 3) and est.std.dtype == torch.float32 and est.mean.device.type == "cuda"
        assert torch.equal(tile.transform(x), got) and torch.equal(tile.apply(x, est), got) and torch.equal(tile.fit_transform(ref)[0], tile.transform(ref)[0])
        one = tile.estimate(x, pooled=True)
        assert one.mean.shape == (1, 3) and torch.equal(tile.apply(x, one), pooled) and torch.equal(tile.apply(x, (one.mean[0], one.std[0])), pooled)
        batch = Reinhard(device=dev, backend="torch_hip").fit(ref)
        assert torch.equal(batch.transform(x), pooled), what      # "batch" after "tile" calls on other engines and on this one:
        assert torch.equal(be.transform(x, rm, rs), pooled) and be.workspace_status() == 0


def test_batch_mode_after_tile_mode_on_one_engine(dev):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP, ReinhardHIP

    x, _, ref = mixed_batch()
    x, ref = x.to(dev), ref.to(dev)
    rb, hb = ReinhardHIP(dev), HistogramMatchingHIP(dev)
    rm, rs = rb.compute_reference_mean_std(ref)
    hists = hb.compute_reference_histograms(ref)
    want_r, want_h = rb.transform(x, rm, rs), hb.transform(x, hists)
    for _ in range(2):
        rb.transform_tiles(x, rm, rs)
        hb.transform_tiles(x, hists)
        assert torch.equal(rb.transform(x, rm, rs), want_r) and rb.workspace_status() == 0
        assert torch.equal(hb.transform(x, hists), want_h) and hb.workspace_status() == 0
    assert rb.transform_tiles(x[:0], rm, rs).shape == (0, 3, 96, 96) and hb.transform_tiles(x[:0], hists).shape == (0, 3, 96, 96)
    mean, std = rb.tile_statistics(x[:0])
    assert mean.shape == (0, 3) and std.shape == (0, 3)


# ------------------------------------------------------------------ workspace etiquette
def test_reinhard_tiles_workspace_etiquette(dev):
    lib = _native.require()
    src = synth.as_dtype(synth.noise_u8((5, 3, 200, 328), 7), torch.float32).to(dev)
    mean = torch.tensor([150.0, 130.0, 120.0], device=dev)
    std = torch.tensor([40.0, 9.0, 12.0], device=dev)
    f32 = _native.DTYPE_CODES[torch.float32]
    stream = _native.stream_ptr(dev)
    shapes = [src, src[:2, :, :64, :96].contiguous(), src[:5, :, :200, :200].contiguous(), src[:1].contiguous()]
    size = max(int(lib.sx_reinhard_tiles_workspace_bytes(f32, x.shape[0], x.shape[2], x.shape[3])) for x in shapes)
    off = int(lib.sx_reinhard_workspace_status_offset())

    def status(ws):
        return int(ws[off:off + 4].view(torch.int32).item())

    def tiles(x, ws):
        out = torch.empty_like(x)
        assert lib.sx_reinhard_transform_tiles(x.data_ptr(), out.data_ptr(), f32, x.shape[0], x.shape[2], x.shape[3], mean.data_ptr(), std.data_ptr(), None, None,
                                               ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def pooled(x, ws, fn):
        out = torch.empty_like(x)
        assert fn(x.data_ptr(), out.data_ptr(), f32, x.shape[0], x.shape[2], x.shape[3], mean.data_ptr(), std.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        return out

    clean = torch.zeros(size, dtype=torch.uint8, device=dev)
    want_tiles = [tiles(x, clean) for x in shapes]
    want_pooled = [pooled(x, clean, lib.sx_reinhard_transform) for x in shapes]
    oracle = reinhard_oracle_tiles(src.cpu(), mean.cpu().numpy(), std.cpu().numpy())
    assert (want_tiles[0].cpu() - oracle).abs().max().item() <= 1e-4
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
    assert torch.equal(tiles(src, ws), want_tiles[0]) and status(ws) == 0          # garbage in: the call clears what it needs ...
    assert torch.equal(pooled(src, ws, lib.sx_reinhard_transform_ready), want_pooled[0]) and status(ws) == 0      # ... and leaves the workspace ready
    for _ in range(2):
        order = list(range(len(shapes))) + list(range(len(shapes)))[::-1]
        for k in order:
            assert torch.equal(tiles(shapes[k], ws), want_tiles[k]) and status(ws) == 0, tuple(shapes[k].shape)
            assert torch.equal(pooled(shapes[k - 1], ws, lib.sx_reinhard_transform_ready), want_pooled[k - 1]) and status(ws) == 0, tuple(shapes[k - 1].shape)


def test_hm_tiles_workspace_etiquette(dev):
    from stainx_amd.backends.torch_hip_backend import HistogramMatchingHIP

    lib = _native.require()
    be = HistogramMatchingHIP(dev)
    src = synth.noise_u8((3, 3, 200, 328), 7).to(dev)
    ref = torch.stack(be.compute_reference_histograms(synth.noise_u8((1, 3, 200, 328), 8).to(dev))).contiguous()
    hists = [r.cpu().numpy() for r in ref]
    u8 = _native.DTYPE_CODES[torch.uint8]
    stream = _native.stream_ptr(dev)
    shapes = [src, src[:2, :, :64, :96].contiguous(), src[:1].contiguous()]
    want_tiles = [hm_oracle_tiles(x.cpu(), hists, 1).to(dev) for x in shapes]
    want_pooled = [torch.from_numpy(so.hm_transform(x.cpu().numpy(), hists)).to(dev) for x in shapes]
    ws = torch.full((max(int(lib.sx_hm_tiles_workspace_bytes(x.shape[0], x.shape[2], x.shape[3])) for x in shapes),), 0xA5, dtype=torch.uint8, device=dev)
    off = int(lib.sx_hm_workspace_status_offset())

    def status():
        return int(ws[off:off + 4].view(torch.int32).item())

    def tiles(x):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_tiles(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), None, None, ws.data_ptr(), ws.numel(), stream) == 0
        return out

    def ready(x):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_ready(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        return out

    assert torch.equal(tiles(src), want_tiles[0]) and status() == 0                # garbage in
    for _ in range(2):
        for k in (0, 1, 2, 2, 1, 0):
            assert torch.equal(ready(shapes[k - 1]), want_pooled[k - 1]) and status() == 0
            assert torch.equal(tiles(shapes[k]), want_tiles[k]) and status() == 0


# ------------------------------------------------------------------ captured graph
def test_apply_stats_in_a_captured_graph_reads_the_statistics_at_replay(dev):
    from stainx_amd.backends.torch_hip_backend import ReinhardHIP

    lib = _native.require()
    be = ReinhardHIP(dev)
    x = synth.as_dtype(synth.he_batch(4, 96, 96, seed0=500, scale_step=0.1), torch.float32).to(dev)
    rm, rs = be.compute_reference_mean_std(synth.reference_tile(96, 96).to(dev))
    first_mean, first_std = be.tile_statistics(x)
    new_mean, new_std = first_mean * 1.02 + 1.0, first_std * 0.9
    mean, std = first_mean.clone(), first_std.clone()
    out = torch.empty_like(x)
    f32 = _native.DTYPE_CODES[torch.float32]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: one launch on one stream
        assert lib.sx_reinhard_apply_stats(x.data_ptr(), out.data_ptr(), f32, 4, 96, 96, mean.data_ptr(), std.data_ptr(), 4, rm.data_ptr(), rs.data_ptr(),
                                           _native.stream_ptr(dev)) == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, be.apply_statistics(x, first_mean, first_std, rm, rs))
    mean.copy_(new_mean)
    std.copy_(new_std)
    graph.replay()
    torch.cuda.synchronize(dev)
    want = be.apply_statistics(x, new_mean, new_std, rm, rs)
    assert torch.equal(out, want) and not torch.equal(want, be.apply_statistics(x, first_mean, first_std, rm, rs))


# ------------------------------------------------------------------ the nn.Module wrapper
def test_tile_mode_passes_through_the_transform_module(dev):
    from stainx_amd import HistogramMatching, Reinhard, StainNormalizerTransform

    x, y, ref = mixed_batch()
    for cls in (Reinhard, HistogramMatching):
        inner = cls(device=dev, backend="torch_hip", statistics="tile")
        module = StainNormalizerTransform(normalizer=inner, reference=ref.to(dev), device=dev)
        a, b = module(x.to(dev)).cpu(), module(y.to(dev)).cpu()
        assert torch.equal(a, inner.transform(x.to(dev)).cpu())
        assert torch.equal(a[[0, 1, 3, 4]], b[[0, 1, 3, 4]])
        assert torch.equal(module(x[3].to(dev)).cpu(), a[3]) or cls is Reinhard      # a CHW tile alone (Reinhard: another grid, another rounding)
        want = reinhard_oracle_tiles(x, *so.reinhard_fit(ref.numpy())) if cls is Reinhard else hm_oracle_tiles(x, so.hm_fit(ref.numpy()), 1)
        assert (a.int() - want.int()).abs().max().item() <= (1 if cls is Reinhard else 0)
