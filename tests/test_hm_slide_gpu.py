"""Slide-level histogram matching on the GPU: ``estimate`` / ``lookup_tables`` / ``apply`` against the existing transforms and against the
numpy restatement of tests/_hm_slide_numpy.py and tests/_masked_numpy.py.  Everything here is integer counting, a fixed-order table and a
lookup, so EVERY comparison is bit for bit (``torch.equal``): there is no tolerance in this file.  The real tiles are those of the
real-tissue fixture (tests/golden/g11_real_images.npz, the images tests/golden/g11_real_tissue.npz was computed from)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import HistogramMatching, HistogramStatistics, _native, synth, tissue_mask
from tests import _hm_slide_numpy as sn
from tests import _masked_numpy as mn
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu

THRESHOLD = 0.8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def unaligned_copy(x: torch.Tensor) -> torch.Tensor:
    """The same values, dense, one element behind an aligned address."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def bits(t: torch.Tensor) -> torch.Tensor:
    views = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
    return t.view(views[t.dtype]) if t.dtype in views else t


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def mixed_tiles() -> torch.Tensor:
    """uint8, (5, 3, 96, 96): three Beer-Lambert tiles with glass stripes (one of them all glass) and two noise tiles."""
    return torch.cat([mn.striped_tiles()[[1, 3, 5]], mn.noise_tiles((2, 3, 96, 96), 11)])


def normalisers(dev, last: bool, ref: torch.Tensor, **kw):
    axis = -1 if last else 1
    ref = ref.permute(0, 2, 3, 1).contiguous() if last else ref
    return [HistogramMatching(device=dev, backend="torch_hip", channel_axis=axis, statistics=s, **kw).fit(ref.to(dev)) for s in ("tile", "batch")]


def layout_of(x: torch.Tensor, last: bool) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous() if last else x


# ------------------------------------------------------------------ 1. identity with the existing paths
@pytest.mark.parametrize("last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["u8", "f16", "bf16", "f32"])
def test_estimate_tables_apply_is_the_existing_transform(dev, name, last):
    dt = TORCH_DTYPES[name]
    ref = synth.reference_tile(96, 96)
    cases = [("mixed_96", mixed_tiles()), ("odd_321x199", synth.noise_u8((3, 3, 321, 199), 21)), ("unaligned", mixed_tiles()[:3])]
    for what, tiles_u8 in cases:
        x = layout_of(synth.as_dtype(tiles_u8, dt), last).to(dev)
        if what == "unaligned":
            x = unaligned_copy(x)
        explicit = tissue_mask(x, 0.6, channel_axis=-1 if last else 1)[0]      # (another cut than the rule's: the explicit mask is what counts)
        for mask_kw, call_mask in (({}, None), ({"mask": "luminosity", "luminosity_threshold": THRESHOLD}, None), ({}, explicit)):
            tile, batch = normalisers(dev, last, synth.as_dtype(ref, dt), **mask_kw)
            for norm, pooled in ((tile, False), (batch, True)):
                want = norm.transform(x, mask=call_mask)
                stats = norm.estimate(x, pooled=pooled, mask=call_mask)
                assert stats.counts.shape == ((1 if pooled else x.shape[0]), 3, 256) and stats.counts.dtype == torch.int64 and stats.counts.device.type == "cuda"
                tables = norm.lookup_tables(stats)
                assert tables.shape == stats.counts.shape and tables.dtype == torch.float32
                got = norm.apply(x, tables, mask=call_mask)
                assert same_bits(got, want), (what, name, last, mask_kw, call_mask is not None, pooled)
                assert same_bits(norm.apply(x, stats, mask=call_mask), want), (what, "statistics as the source")      # the two-launch form
                if pooled:
                    assert same_bits(norm.apply(x, tables[0], mask=call_mask), want), (what, "a (3, 256) source")


def test_estimate_needs_no_fit_and_accepts_f64(dev):
    x = synth.as_dtype(mixed_tiles(), torch.float64).to(dev)
    stats = HistogramMatching(device=dev, backend="torch_hip").estimate(x)
    assert torch.equal(stats.counts.cpu(), torch.from_numpy(sn.bincounts(x.cpu().numpy())))
    norm = HistogramMatching(device=dev, backend="torch_hip", statistics="tile").fit(synth.reference_tile(96, 96).to(dev))
    assert same_bits(norm.apply(x, norm.lookup_tables(stats)), norm.transform(x))


# ------------------------------------------------------------------ 2. estimate
def estimate_cases():
    yield "noise_5x200x328", mn.noise_tiles()
    yield "real_256", mn.real_crops(256)
    yield "real_512_test_5", mn.real_crops(512)[5:6]
    yield "odd_2x33x47", synth.noise_u8((2, 3, 33, 47), 143)


@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_estimate_counts_are_the_bincounts(dev, name):
    dt = TORCH_DTYPES[name]
    for what, tiles_u8 in estimate_cases():
        src = synth.as_dtype(tiles_u8, dt)
        want = torch.from_numpy(sn.bincounts(mn.oracle_input(src)))
        n, _, h, w = src.shape
        for last in (False, True):
            norm = HistogramMatching(device=dev, backend="torch_hip", channel_axis=-1 if last else 1)
            x = layout_of(src, last).to(dev)
            for form in (x, unaligned_copy(x)):
                per_tile, pooled = norm.estimate(form), norm.estimate(form, pooled=True)
                assert torch.equal(per_tile.counts.cpu(), want), (what, name, last)
                assert torch.equal(per_tile.pixels.cpu(), torch.full((n,), h * w, dtype=torch.int64))
                assert torch.equal(pooled.counts.cpu(), want.sum(0, keepdim=True)), (what, name, last)
                assert pooled.pixels.cpu().tolist() == [n * h * w]
                assert norm._get_backend_impl().workspace_status() == 0


@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_masked_estimate_counts_the_tissue(dev, name):
    dt = TORCH_DTYPES[name]
    for what, tiles_u8 in list(estimate_cases()) + [("stripes", mn.striped_tiles())]:
        src = synth.as_dtype(tiles_u8, dt)
        n = src.shape[0]
        for last in (False, True):
            axis = -1 if last else 1
            x = layout_of(src, last).to(dev)
            mask, tissue = tissue_mask(x, THRESHOLD, channel_axis=axis)
            m = mask.cpu().numpy() != 0
            images = mn.oracle_input(layout_of(src, last))
            want_tiles = torch.from_numpy(np.stack([mn.hm_counts(images[t:t + 1], m[t:t + 1], axis) for t in range(n)]))
            want_pooled = torch.from_numpy(mn.hm_counts(images, m, axis)[None])
            rule = HistogramMatching(device=dev, backend="torch_hip", channel_axis=axis, mask="luminosity", luminosity_threshold=THRESHOLD)
            plain = HistogramMatching(device=dev, backend="torch_hip", channel_axis=axis)
            for norm, call_mask in ((rule, None), (plain, mask), (plain, "luminosity")):
                per_tile, pooled = norm.estimate(x, mask=call_mask), norm.estimate(x, pooled=True, mask=call_mask)
                assert torch.equal(per_tile.counts.cpu(), want_tiles), (what, name, last)
                assert torch.equal(per_tile.pixels, tissue) and torch.equal(per_tile.pixels.cpu(), torch.from_numpy(m.reshape(n, -1).sum(1)))
                assert torch.equal(per_tile.pixels, per_tile.counts.sum(2)[:, 0]) and torch.equal(per_tile.pixels, per_tile.counts.sum(2)[:, 2])
                assert torch.equal(pooled.counts.cpu(), want_pooled), (what, name, last)
                assert pooled.pixels.cpu().tolist() == [int(m.sum())] and pooled.pixels.item() == pooled.counts[0, 1].sum().item()
            # ... and they are the histograms the masked transform itself counted with the same arguments
            be = plain._get_backend_impl()
            ref = [torch.full((256,), 1.0 / 256, device=dev)] * 3
            for per_tile in (True, False):
                _, tables = be.transform_masked(x, ref, None, THRESHOLD, per_tile=per_tile, return_tables=True)
                got = rule.estimate(x, pooled=not per_tile)
                assert torch.equal(got.counts, tables["counts"].long()) and torch.equal(got.pixels, tables["tissue"])


# ------------------------------------------------------------------ 3. tables
def test_lookup_tables_are_the_oracles_row_by_row(dev):
    ref_tile = synth.reference_tile(128, 128)
    norm = HistogramMatching(device=dev, backend="torch_hip").fit(ref_tile.to(dev))
    hists = [h.cpu().numpy() for h in norm._ref_histograms_256]
    x = torch.cat([mn.real_crops(256), mn.noise_tiles((2, 3, 256, 256), 3)]).to(dev)
    counted = norm.estimate(x)
    one_bin = torch.zeros((3, 3, 256), dtype=torch.int64)
    one_bin[0, :, 0], one_bin[1, :, 255], one_bin[2, 0, 17], one_bin[2, 1, 200], one_bin[2, 2, 128] = 4096, 4096, 9, 9, 9
    one_bin_pixels = torch.tensor([4096, 4096, 9])
    g = torch.Generator().manual_seed(9)
    big = torch.randint(0, 1 << 36, (4, 3, 256), generator=g) + (1 << 32)      # beyond 2^32 per bin, written by hand
    big[1] = (1 << 40) + torch.arange(256) * (1 << 33)
    big[2, :, 100:] = 0
    big[2, :, :100] += 1 << 44
    big_pixels = big.sum(2)[:, 0].clone()
    big[3] = big[0]
    big_pixels[3] = big_pixels[0] * 3      # (a divisor that is not the sum: the table never reaches 255's running sum)
    cases = {"counted": (counted.counts.cpu(), counted.pixels.cpu()), "pooled": tuple(t.cpu() for t in HistogramStatistics.pool(counted)), "one_bin": (one_bin, one_bin_pixels),
             "beyond_2^32": (big, big_pixels)}
    for what, (counts, pixels) in cases.items():
        want = sn.tables(counts.numpy(), pixels.numpy(), hists)
        assert np.isfinite(want).all() and (np.diff(want, axis=2) >= 0).all(), what      # the oracle stays finite and monotone there
        got = norm.lookup_tables(HistogramStatistics(counts.to(dev), pixels.to(dev)))
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert torch.equal(bits(got.cpu()), bits(torch.from_numpy(want))), (what, float((got.cpu() - torch.from_numpy(want)).abs().max()))
    assert counted.counts.max().item() < 1 << 32 <= min(big[0].min().item(), big[1].min().item())


def test_a_set_without_pixels_gets_the_identity_table(dev):
    norm = HistogramMatching(device=dev, backend="torch_hip").fit(synth.reference_tile(64, 64).to(dev))
    x = mn.striped_tiles().to(dev)      # the last tile is all glass
    stats = norm.estimate(x, mask="luminosity")
    assert stats.pixels[5].item() == 0 and stats.pixels[0].item() > 0
    tables = norm.lookup_tables(stats)
    identity = torch.arange(256, dtype=torch.float32, device=dev)
    for c in range(3):
        assert torch.equal(tables[5, c], identity)
    assert not torch.equal(tables[0, 0], identity)
    zero = HistogramStatistics(torch.zeros((2, 3, 256), dtype=torch.int64, device=dev), torch.zeros((2,), dtype=torch.int64, device=dev))
    assert torch.equal(norm.lookup_tables(zero), identity.expand(2, 3, 256))
    # ... which leaves uint8 grey levels where they are
    assert torch.equal(norm.apply(x[5:6], tables[5:6]), x[5:6])


# ------------------------------------------------------------------ 4. accumulation
@pytest.mark.parametrize("name", ["u8", "bf16"])
def test_histograms_of_batches_add_up_to_the_histogram_of_the_slide(dev, name):
    dt = TORCH_DTYPES[name]
    x = synth.as_dtype(torch.cat([mn.real_crops(256), mixed_tiles().repeat(1, 1, 3, 3)[:, :, :256, :256]]), dt).to(dev)
    ref = synth.as_dtype(synth.reference_tile(128, 128), dt).to(dev)
    for mask_kw in ({}, {"mask": "luminosity", "luminosity_threshold": THRESHOLD}):
        batch = HistogramMatching(device=dev, backend="torch_hip", statistics="batch", **mask_kw).fit(ref)
        whole = batch.estimate(x, pooled=True)
        for k in (1, 4, 10):
            parts = HistogramStatistics.pool(batch.estimate(x[:k], pooled=True), batch.estimate(x[k:], pooled=True))
            assert torch.equal(parts.counts, whole.counts) and torch.equal(parts.pixels, whole.pixels), (name, mask_kw, k)
            per_tile = HistogramStatistics.pool(batch.estimate(x[:k]), batch.estimate(x[k:]))      # sets per tile, summed by pool
            assert torch.equal(per_tile.counts, whole.counts) and torch.equal(per_tile.pixels, whole.pixels)
        table = batch.lookup_tables(parts)
        want = batch.transform(x)
        assert same_bits(batch.apply(x, table), want), (name, mask_kw)
        assert same_bits(torch.cat([batch.apply(x[:3], table), batch.apply(x[3:], table)]), want)      # batch by batch, one table


# ------------------------------------------------------------------ 5. a foreign source, 6. independence
@pytest.mark.parametrize("last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["u8", "f32", "bf16"])
def test_foreign_tables_against_the_numpy_lookup(dev, name, last):
    dt = TORCH_DTYPES[name]
    axis = -1 if last else 1
    src = synth.as_dtype(torch.cat([mn.real_crops(128), mn.noise_tiles((2, 3, 128, 128), 5)]), dt)
    n = src.shape[0]
    norm = normalisers(dev, last, synth.as_dtype(synth.reference_tile(128, 128), dt))[0]
    hists = [h.cpu().numpy() for h in norm._ref_histograms_256]
    x = layout_of(src, last).to(dev)
    images = mn.oracle_input(layout_of(src, last))
    counts = sn.bincounts(images, axis)
    pixels = np.full((n,), 128 * 128, dtype=np.int64)
    tables = norm.lookup_tables(norm.estimate(x))
    assert torch.equal(bits(tables.cpu()), bits(torch.from_numpy(sn.tables(counts, pixels, hists))))
    luts = tables.cpu().numpy()
    # n_sources = 1: tile A's table on every tile
    for a in (0, n - 1):
        want = mn.oracle_cast(sn.lookup(images, luts[a:a + 1], axis), dt)
        assert same_bits(norm.apply(x, tables[a:a + 1]).cpu(), want), (name, last, a)
    # n_sources = N: the tables of a permuted batch -- tile t takes the table of tile perm[t]
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4][:n]) if n == 8 else torch.roll(torch.arange(n), 1)
    want = mn.oracle_cast(sn.lookup(images, luts[perm.numpy()], axis), dt)
    got = norm.apply(x, tables[perm.to(dev)])
    assert same_bits(got.cpu(), want), (name, last)
    assert not same_bits(got, norm.transform(x))
    for form in (unaligned_copy(x),):      # the single-element path gives the same bits
        assert same_bits(norm.apply(form, tables[perm.to(dev)]).cpu(), want)


def test_a_tile_and_its_row_change_no_other_tile(dev):
    norm = HistogramMatching(device=dev, backend="torch_hip", statistics="tile").fit(synth.reference_tile(96, 96).to(dev))
    for dt in (torch.uint8, torch.float32):
        x = synth.as_dtype(mixed_tiles(), dt).to(dev)
        tables = norm.lookup_tables(norm.estimate(x))
        base = norm.apply(x, tables)
        for j in (0, 2, 4):
            x2, t2 = x.clone(), tables.clone()
            x2[j] = synth.as_dtype(synth.noise_u8((1, 3, 96, 96), 900 + j), dt).to(dev)[0]
            t2[j] = tables[(j + 1) % 5].flip(1)
            out = norm.apply(x2, t2)
            others = [t for t in range(5) if t != j]
            assert same_bits(out[others], base[others]) and not same_bits(out[j], base[j]), (dt, j)
            mask = tissue_mask(x2, THRESHOLD)[0]
            masked, masked_base = norm.apply(x2, t2, mask=mask), norm.apply(x, tables, mask=tissue_mask(x, THRESHOLD)[0])
            assert same_bits(masked[others], masked_base[others]), (dt, j, "masked")


# ------------------------------------------------------------------ 7. one launch, device-side reads
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_apply_tables_in_a_captured_graph_reads_tables_and_mask_at_replay(dev, masked):
    lib = _native.require()
    norm = HistogramMatching(device=dev, backend="torch_hip", statistics="tile").fit(synth.reference_tile(96, 96).to(dev))
    be = norm._get_backend_impl()
    x = synth.as_dtype(mixed_tiles()[:4], torch.float32).to(dev)
    first_tables = norm.lookup_tables(norm.estimate(x))
    new_tables = first_tables.flip(0).contiguous() * 0.5 + 3.0
    first_mask = tissue_mask(x, THRESHOLD)[0]
    new_mask = first_mask.clone()
    new_mask[:, :48] = 0
    tables, mask = first_tables.clone(), first_mask.clone()
    out = torch.empty_like(x)
    f32 = _native.DTYPE_CODES[torch.float32]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # a linear capture: one launch on one stream; the call takes no workspace at all
        if masked:
            assert lib.sx_hm_apply_tables_masked(x.data_ptr(), out.data_ptr(), f32, 4, 96, 96, 0, tables.data_ptr(), 4, mask.data_ptr(), THRESHOLD, _native.stream_ptr(dev)) == 0
        else:
            assert lib.sx_hm_apply_tables(x.data_ptr(), out.data_ptr(), f32, 4, 96, 96, 0, tables.data_ptr(), 4, _native.stream_ptr(dev)) == 0

    def eager(t, m):
        return be.apply_tables_masked(x, t, m, THRESHOLD) if masked else be.apply_tables(x, t)

    graph.replay()
    torch.cuda.synchronize(dev)
    first = eager(first_tables, first_mask)
    assert same_bits(out, first)
    tables.copy_(new_tables)
    mask.copy_(new_mask)
    graph.replay()
    torch.cuda.synchronize(dev)
    want = eager(new_tables, new_mask)
    assert same_bits(out, want) and not same_bits(want, first)
    if masked:
        assert same_bits(out[:, :, :48], x[:, :, :48])      # the new mask's background, read at replay


# ------------------------------------------------------------------ 8. workspace etiquette of estimate
def test_estimate_workspace_etiquette(dev):
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

    want_masked = [torch.from_numpy(mn.hm_transform(x.cpu().numpy(), hists, rule(x), True)).to(dev) for x in shapes]
    want_tiles = [torch.from_numpy(np.concatenate([so.hm_transform(x[i:i + 1].cpu().numpy(), hists) for i in range(x.shape[0])])).to(dev) for x in shapes]
    want_pooled = [torch.from_numpy(so.hm_transform(x.cpu().numpy(), hists)).to(dev) for x in shapes]
    want_counts = [torch.from_numpy(sn.bincounts(x.cpu().numpy())).to(dev) for x in shapes]
    want_tissue = [torch.from_numpy(np.stack([mn.hm_counts(x[t:t + 1].cpu().numpy(), rule(x)[t:t + 1]) for t in range(x.shape[0])])).to(dev) for x in shapes]
    size = max(max(int(lib.sx_hm_masked_workspace_bytes(x.shape[0], x.shape[2], x.shape[3])), int(lib.sx_hm_tiles_workspace_bytes(x.shape[0], x.shape[2], x.shape[3]))) for x in shapes)
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
    off = int(lib.sx_hm_workspace_status_offset())

    def status():
        return int(ws[off:off + 4].view(torch.int32).item())

    def estimate(x, per_tile, masked):
        sets = x.shape[0] if per_tile else 1
        counts = torch.full((sets, 3, 256), -1, dtype=torch.int64, device=dev)
        pixels = torch.full((sets,), -1, dtype=torch.int64, device=dev)
        if masked:
            rc = lib.sx_hm_estimate_masked(x.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, per_tile, None, THRESHOLD, counts.data_ptr(), pixels.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        else:
            rc = lib.sx_hm_estimate(x.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, per_tile, counts.data_ptr(), pixels.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, _native.last_error()
        assert torch.equal(pixels, counts.sum(2)[:, 1])
        return counts

    def masked(x):
        out = torch.empty_like(x)
        assert lib.sx_hm_transform_masked(x.data_ptr(), out.data_ptr(), u8, x.shape[0], x.shape[2], x.shape[3], 0, ref.data_ptr(), None, THRESHOLD, 1, None, None, None,
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

    def check(k, per_tile, with_mask):
        got = estimate(shapes[k], per_tile, with_mask)
        want = (want_tissue if with_mask else want_counts)[k]
        assert torch.equal(got, want if per_tile else want.sum(0, keepdim=True)) and status() == 0, (k, per_tile, with_mask)

    check(0, 1, False)                                                                     # garbage in
    assert torch.equal(ready(src), want_pooled[0]) and status() == 0                       # READY out
    ws.fill_(0x5A)
    check(0, 0, True)                                                                      # garbage in, the masked layout
    assert torch.equal(ready(src), want_pooled[0]) and status() == 0
    ws.fill_(0xC3)
    check(1, 0, False)                                                                     # garbage in, a pooled call
    assert torch.equal(ready(shapes[1]), want_pooled[1]) and status() == 0
    for _ in range(2):
        for k in (0, 1, 2, 2, 1, 0):
            for per_tile in (1, 0):
                for with_mask in (False, True):
                    check(k, per_tile, with_mask)
                    assert torch.equal(ready(shapes[k - 1]), want_pooled[k - 1]) and status() == 0
                check(k - 1, per_tile, False)
                assert torch.equal(tiles(shapes[k - 2]), want_tiles[k - 2]) and status() == 0
                check(k - 2, per_tile, True)
                assert torch.equal(masked(shapes[k]), want_masked[k]) and status() == 0
            check(k, 1, True)
            check(k, 0, False)                                                              # two estimates in a row


# ------------------------------------------------------------------ 9. masked background
@pytest.mark.parametrize("last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["u8", "f16", "bf16", "f32", "f64"])
def test_masked_apply_copies_the_background_and_matches_the_unmasked_tissue(dev, name, last):
    dt = TORCH_DTYPES[name]
    axis = -1 if last else 1
    norm = normalisers(dev, last, synth.as_dtype(synth.reference_tile(96, 96), dt))[0]
    for what, tiles_u8 in (("mixed", mixed_tiles()), ("odd_33x47", torch.cat([synth.noise_u8((2, 3, 33, 47), 143), synth.background_stripes(synth.he_batch(2, 33, 47, seed0=70))]))):
        src = synth.as_dtype(tiles_u8, dt)
        if dt != torch.uint8:
            src = src + (torch.rand(src.shape, generator=torch.Generator().manual_seed(3)) * 2e-3).to(dt)      # floats off the 8-bit grid: a quantised copy would show
        x = layout_of(src, last).to(dev)
        tables = norm.lookup_tables(norm.estimate(x, mask="luminosity"))
        plain = norm.apply(x, tables)
        rule_mask = tissue_mask(x, THRESHOLD, channel_axis=axis)[0]
        other = (torch.rand(rule_mask.shape, generator=torch.Generator().manual_seed(4)) < 0.5).to(dev)      # a bool mask unrelated to the pixels
        for call_mask, m in (("luminosity", rule_mask != 0), (rule_mask, rule_mask != 0), (other, other)):
            got = norm.apply(x, tables, mask=call_mask)
            tissue = (m.unsqueeze(-1) if last else m.unsqueeze(1)).expand_as(x)
            assert torch.equal(bits(got)[~tissue], bits(x)[~tissue]), (what, name, last, "background")
            assert torch.equal(bits(got)[tissue], bits(plain)[tissue]), (what, name, last, "tissue")
            one = norm.apply(x, tables[1:2], mask=call_mask)      # one source for the batch
            assert torch.equal(bits(one)[~tissue], bits(x)[~tissue]) and torch.equal(bits(one)[tissue], bits(norm.apply(x, tables[1:2]))[tissue])
        assert 0 < int((rule_mask != 0).sum()) < rule_mask.numel()
