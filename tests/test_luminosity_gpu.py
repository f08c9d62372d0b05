"""Luminosity standardisation on the GPU.

The percentile is checked EXACTLY, with no tolerance and no restatement, against a kernel that already exists: sx_tissue_mask_tiles with
the returned Y_p as the per-tile cut counts the pixels with Y < Y_p (c0), with nextafter(Y_p, +inf) those with Y <= Y_p (c1), and the
k-th smallest Y of S is Y_p iff c0 < k <= c1, k from ``pixels`` and the rank rule.  The apply pass is checked against the float64
restatement (tests/_luminosity_numpy.py) fed the GPU's own Y_p, with the project's tolerances for this conversion chain."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from stainx_amd import LuminosityEstimate, LuminosityStandardizer, _native, synth
from tests import _luminosity_numpy as ln
from tests.conftest import TORCH_DTYPES

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 4), (2, 33, 47), (3, 30, 30), (3, 150, 203)]      # (3, 150, 203): two 16 384-pixel work items with a ragged end, a width that is no multiple of 4
PERCENTILES = (0.5, 50.0, 95.0, 100.0)
DTYPES = ["u8", "f16", "bf16", "f32", "f64"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def standardizers():
    return {p: LuminosityStandardizer(p) for p in PERCENTILES}


@pytest.fixture(scope="module")
def real_u8():
    return torch.from_numpy(ln.real_images())


def counts_below(x: torch.Tensor, cuts: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    """(N,) int64: per tile the pixels of S with Y < cut, by sx_tissue_mask_tiles called raw (its mask output ANDed with ``mask``)."""
    lib = _native.require()
    n, _, h, w = x.shape
    out = torch.full((n, h, w), 7, dtype=torch.uint8, device=x.device)
    rc = lib.sx_tissue_mask_tiles(x.data_ptr(), _native.DTYPE_CODES[x.dtype], n, h, w, 0, cuts.contiguous().data_ptr(), out.data_ptr(), None, _native.stream_ptr(x.device))
    assert rc == 0, _native.last_error()
    inside = out != 0
    if mask is not None:
        inside &= mask != 0
    return inside.flatten(1).sum(dim=1)


def assert_bracket(x: torch.Tensor, est: LuminosityEstimate, percentile: float, pooled: bool, mask: torch.Tensor | None, set_sizes: torch.Tensor, what) -> None:
    """c0 < k <= c1 and pixels == |S| for every row.  ``set_sizes``: (N,) int64 |S| per tile."""
    n = x.shape[0]
    rows = 1 if pooled else n
    assert est.luminance.shape == (rows,) and est.luminance.dtype == torch.float32 and est.pixels.shape == (rows,) and est.pixels.dtype == torch.int64, what
    cuts = est.luminance.expand(n).contiguous() if pooled else est.luminance
    c0 = counts_below(x, cuts, mask)
    c1 = counts_below(x, torch.nextafter(cuts, torch.full_like(cuts, float("inf"))), mask)
    if pooled:
        c0, c1, set_sizes = c0.sum(0, keepdim=True), c1.sum(0, keepdim=True), set_sizes.sum(0, keepdim=True)
    got = torch.stack([est.pixels, c0, c1, set_sizes.to(c0.device)]).cpu().tolist()
    lum = est.luminance.cpu().tolist()
    for row in range(rows):
        pixels, below, upto, size = (got[i][row] for i in range(4))
        assert pixels == size, (what, row, pixels, size)
        if size == 0:
            assert np.isnan(lum[row]), (what, row, lum[row])
            continue
        k = ln.rank(pixels, percentile)
        assert below < k <= upto, (what, row, lum[row], below, k, upto)


def unaligned(x: torch.Tensor) -> torch.Tensor:
    """The same values one element off the allocation's alignment."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def inputs_u8(shape: tuple[int, int, int], real: torch.Tensor) -> dict[str, torch.Tensor]:
    n, h, w = shape
    out = {"random": synth.noise_u8((n, 3, h, w), 7 + h), "he": synth.he_batch(n, h, w, seed0=300, scale_step=0.1)}
    out["constant"] = torch.full((n, 3, h, w), 181, dtype=torch.uint8)
    glass = synth.noise_u8((n, 3, h, w), 11 + w)      # 97 % one glass value
    gen = torch.Generator().manual_seed(5)
    is_glass = torch.rand(n, 1, h, w, generator=gen) < 0.97
    glass = torch.where(is_glass, torch.tensor([243, 241, 244], dtype=torch.uint8).view(1, 3, 1, 1), glass)
    out["glass97"] = glass
    if (h, w) == (150, 203):
        out["real"] = real[:n, :, 300:450, 400:603].contiguous()      # a 150-row crop of the real fixture
    return out


def some_mask(n: int, h: int, w: int, dev) -> torch.Tensor:
    gen = torch.Generator().manual_seed(3 * h + w)
    mask = (torch.rand(n, h, w, generator=gen) < 0.6).to(torch.uint8)
    mask.view(-1)[0] = 1      # (never empty)
    return mask.to(dev)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", DTYPES)
def test_percentile_is_bracketed_by_the_rule_kernel(dev, standardizers, real_u8, name, shape):
    n, h, w = shape
    mask = some_mask(n, h, w, dev)
    full = torch.full((n,), h * w, dtype=torch.int64)
    masked_sizes = mask.flatten(1).sum(dim=1).cpu()
    for tag, tiles in inputs_u8(shape, real_u8).items():
        x = synth.as_dtype(tiles, TORCH_DTYPES[name]).to(dev)
        for percentile, std in standardizers.items():
            for pooled in (False, True):
                assert_bracket(x, std.estimate(x, pooled=pooled), percentile, pooled, None, full, (tag, name, shape, percentile, pooled))
                assert_bracket(x, std.estimate(x, pooled=pooled, mask=mask), percentile, pooled, mask, masked_sizes, (tag, name, shape, percentile, pooled, "mask"))
        assert_bracket(x, standardizers[95.0].estimate(x, mask=mask.bool()), 95.0, False, mask, masked_sizes, (tag, name, shape, "bool mask"))


@pytest.mark.parametrize("name", DTYPES)
def test_unaligned_view(dev, standardizers, name):
    """900 pixels per tile: whole packs from an aligned address, single elements from this view -- the same rows, bit for bit."""
    x = synth.as_dtype(synth.he_batch(3, 30, 30, seed0=40, scale_step=0.1), TORCH_DTYPES[name]).to(dev)
    off = unaligned(x)
    mask = some_mask(3, 30, 30, dev)
    off_mask = unaligned(mask)
    full = torch.full((3,), 900, dtype=torch.int64)
    for percentile, std in standardizers.items():
        for pooled in (False, True):
            want, got = std.estimate(x, pooled=pooled), std.estimate(off, pooled=pooled)
            assert_bracket(off, got, percentile, pooled, None, full, (name, percentile, pooled))
            assert torch.equal(got.luminance, want.luminance) and torch.equal(got.pixels, want.pixels)
            want, got = std.estimate(x, pooled=pooled, mask=mask), std.estimate(off, pooled=pooled, mask=off_mask)
            assert torch.equal(got.luminance, want.luminance) and torch.equal(got.pixels, want.pixels)
    want = standardizers[95.0](x)
    assert torch.equal(standardizers[95.0](off), want)


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_two_level_tile_flips_at_the_rank(dev, standardizers, shape):
    """Exactly k - 1 dark pixels: the k-th smallest is bright.  Exactly k: it is dark."""
    n, h, w = shape
    pixels = h * w
    dark, bright = torch.tensor([40, 60, 50], dtype=torch.uint8), torch.tensor([230, 228, 233], dtype=torch.uint8)
    one = LuminosityStandardizer(100.0)
    y_dark = one.estimate(dark.view(1, 3, 1, 1).to(dev)).luminance
    y_bright = one.estimate(bright.view(1, 3, 1, 1).to(dev)).luminance
    assert y_dark.item() < y_bright.item()
    full = torch.full((1,), pixels, dtype=torch.int64)
    for percentile, std in standardizers.items():
        k = ln.rank(pixels, percentile)
        for n_dark, want in ((k - 1, y_bright), (k, y_dark)):
            gen = torch.Generator().manual_seed(n_dark)
            where = torch.randperm(pixels, generator=gen)[:n_dark]
            tile = bright.view(3, 1).repeat(1, pixels)
            tile[:, where] = dark.view(3, 1)
            for name in ("u8", "f32"):
                x = synth.as_dtype(tile.view(1, 3, h, w), TORCH_DTYPES[name]).to(dev)
                est = std.estimate(x)
                assert_bracket(x, est, percentile, False, None, full, (shape, percentile, n_dark, name))
                if name == "u8":
                    assert torch.equal(est.luminance, want), (shape, percentile, n_dark)


def test_grey_ramp_of_consecutive_floats(dev, standardizers):
    """900 consecutive float32 values below 0.04045 as grey pixels: the keys differ in the last radix digit only."""
    base = torch.tensor([0.02], dtype=torch.float32).view(torch.int32).item()
    values = (base + torch.randperm(900, generator=torch.Generator().manual_seed(9)).to(torch.int32)).view(torch.float32)
    assert values.max().item() < 0.04045
    x = values.view(1, 1, 30, 30).repeat(1, 3, 1, 1).contiguous().to(dev)
    full = torch.full((1,), 900, dtype=torch.int64)
    seen = set()
    for percentile, std in standardizers.items():
        est = std.estimate(x)
        assert_bracket(x, est, percentile, False, None, full, percentile)
        seen.add(est.luminance.item())
    assert len(seen) == 4
    bits = sorted(torch.tensor(sorted(seen), dtype=torch.float32).view(torch.int32).tolist())
    assert bits[-1] - bits[0] < 1024 * 4      # (all four answers share the leading 22 key bits or nearly so: the last pass decides)


@pytest.mark.parametrize("name", DTYPES)
def test_alone_in_a_batch_and_pooled_one_tile(dev, standardizers, real_u8, name):
    x = synth.as_dtype(real_u8[:3, :, 300:450, 400:603].contiguous(), TORCH_DTYPES[name]).to(dev)
    mask = some_mask(3, 150, 203, dev)
    for percentile, std in standardizers.items():
        batch, batch_m = std.estimate(x), std.estimate(x, mask=mask)
        for i in range(3):
            alone, pooled = std.estimate(x[i:i + 1]), std.estimate(x[i:i + 1], pooled=True)
            assert torch.equal(alone.luminance, batch.luminance[i:i + 1]) and torch.equal(alone.pixels, batch.pixels[i:i + 1])
            assert torch.equal(pooled.luminance, alone.luminance) and torch.equal(pooled.pixels, alone.pixels)
            alone_m = std.estimate(x[i:i + 1], mask=mask[i:i + 1])
            assert torch.equal(alone_m.luminance, batch_m.luminance[i:i + 1]) and torch.equal(alone_m.pixels, batch_m.pixels[i:i + 1])
            chw = std.estimate(x[i])      # (3, H, W)
            assert torch.equal(chw.luminance, alone.luminance)


def test_nan_pixels_are_not_in_the_set(dev, standardizers):
    x = synth.as_dtype(synth.he_batch(2, 33, 47, seed0=70, scale_step=0.1), torch.float32).to(dev)
    holes = torch.zeros(2, 33, 47, dtype=torch.bool, device=dev)
    holes.view(2, -1)[0, [3, 500, 501, 1550]] = True
    holes.view(2, -1)[1, [0, 777]] = True
    with_nan = x.clone()
    with_nan[:, 1][holes] = float("nan")      # (one channel is enough: Y is NaN)
    keep = (~holes).to(torch.uint8)
    sizes = keep.flatten(1).sum(dim=1).cpu()
    for percentile, std in standardizers.items():
        for pooled in (False, True):
            got = std.estimate(with_nan, pooled=pooled)
            for reference in (std.estimate(x, pooled=pooled, mask=keep), std.estimate(with_nan, pooled=pooled, mask=keep)):
                assert torch.equal(got.luminance, reference.luminance) and torch.equal(got.pixels, reference.pixels)
            assert_bracket(x, got, percentile, pooled, keep, sizes, (percentile, pooled))
    out = standardizers[95.0](with_nan)      # (what a NaN pixel becomes is unspecified: it only must not fault, and the others are as without it)
    want = standardizers[95.0].apply(x, standardizers[95.0].estimate(with_nan))
    assert torch.equal(out[(~holes).unsqueeze(1).expand_as(out)], want[(~holes).unsqueeze(1).expand_as(out)])


def test_empty_mask_gives_nan_and_zero_pixels(dev, standardizers):
    x = synth.he_batch(3, 30, 30, seed0=80).to(dev)
    mask = torch.ones(3, 30, 30, dtype=torch.uint8, device=dev)
    mask[1] = 0
    std = standardizers[95.0]
    est = std.estimate(x, mask=mask)
    assert torch.isnan(est.luminance).tolist() == [False, True, False] and est.pixels.tolist() == [900, 0, 900]
    assert torch.isnan(est.lightness).tolist() == [False, True, False]
    pooled = std.estimate(x, pooled=True, mask=torch.zeros_like(mask))
    assert torch.isnan(pooled.luminance).all() and pooled.pixels.tolist() == [0]
    out = std(x, mask=mask)
    assert torch.equal(out[1], x[1]) and not torch.equal(out[0], x[0])      # (the tile without an estimate is copied through)


@pytest.mark.parametrize("name", DTYPES)
def test_apply_rows_and_copy_through(dev, standardizers, name):
    dt = TORCH_DTYPES[name]
    std = standardizers[95.0]
    for shape in ((3, 30, 30), (2, 33, 47)):
        n, h, w = shape
        x = synth.as_dtype(synth.he_batch(n, h, w, seed0=90, scale_step=0.1), dt).to(dev)
        one = std.estimate(x[:1])
        out = std.apply(x, one)
        assert out.dtype == dt and out.shape == x.shape and out.data_ptr() != x.data_ptr()
        assert torch.equal(out, std.apply(x, one.luminance.repeat(n)))      # one row against n equal rows
        assert torch.equal(out, std.apply(x, LuminosityEstimate(one.luminance.repeat(n), one.pixels.repeat(n))))
        assert torch.equal(std.apply(x[0], one), out[0])      # (3, H, W) gains and loses the batch axis
        # the copy-through: a NaN row, a black percentile; row by row
        assert torch.equal(std.apply(x, torch.tensor([float("nan")], device=dev)), x)
        assert torch.equal(std.apply(x, torch.tensor([0.0], device=dev)), x)
        rows = one.luminance.repeat(n)
        rows[n - 1] = float("nan")
        mixed = std.apply(x, rows)
        assert torch.equal(mixed[n - 1], x[n - 1]) and torch.equal(mixed[:n - 1], out[:n - 1])
        black = torch.zeros_like(x)
        assert torch.equal(std(black), black)      # a black tile: L_p = 0
        # forward is estimate then apply, per tile and pooled
        assert torch.equal(std(x), std.apply(x, std.estimate(x)))
        assert torch.equal(std.standardize(x), std(x))
        batch = LuminosityStandardizer(95.0, statistics="batch")
        assert torch.equal(batch(x), batch.apply(x, batch.estimate(x, pooled=True)))
        mask = some_mask(n, h, w, dev)
        assert torch.equal(std(x, mask=mask), std.apply(x, std.estimate(x, mask=mask)))


def test_percentile_100_whitens_nothing_below_the_maximum(dev, real_u8):
    """percentile = 100: no output pixel whose input Y lies below Y_p has all three channels at white, unless the restatement says so."""
    std = LuminosityStandardizer(100.0)
    tiles = torch.cat([real_u8[:2, :, 300:450, 400:603], synth.he_batch(1, 150, 203, seed0=5)]).contiguous()
    for name in ("u8", "f32"):
        x = synth.as_dtype(tiles, TORCH_DTYPES[name]).to(dev)
        est = std.estimate(x)
        out = std.apply(x, est)
        lib = _native.require()
        below = torch.empty((3, 150, 203), dtype=torch.uint8, device=dev)
        assert lib.sx_tissue_mask_tiles(x.data_ptr(), _native.DTYPE_CODES[x.dtype], 3, 150, 203, 0, est.luminance.data_ptr(), below.data_ptr(), None, _native.stream_ptr(dev)) == 0
        white = 255 if name == "u8" else 1.0
        got = ((out == white).all(dim=1) & (below != 0)).cpu().numpy()
        ref = ln.standardize_unit(x.cpu().numpy(), est.luminance.cpu().numpy())
        ref_white = (ln.to_levels(ref) == 255).all(axis=1) if name == "u8" else (ref == 1.0).all(axis=1)
        assert not (got & ~ref_white).any(), (name, int((got & ~ref_white).sum()))


def test_captured_forward_replays_on_new_pixels(dev):
    a = synth.he_batch(3, 150, 203, seed0=21, scale_step=0.1).to(dev)
    b = synth.he_batch(3, 150, 203, seed0=22, scale_step=0.2).to(dev)
    for statistics in ("tile", "batch"):
        std = LuminosityStandardizer(95.0, statistics=statistics)
        x = a.clone()
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            std(x)      # (warm-up on the capture stream: its workspace exists before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = std(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, std(a))
        x.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, std(b)) and not torch.equal(out, std(a))


# ------------------------------------------------------------------ the apply pass against the restatement
def restatement_inputs(real: torch.Tensor) -> dict[str, torch.Tensor]:
    dark = (synth.noise_u8((2, 3, 33, 47), 17).float() * 0.25 + 50).round().to(torch.uint8)      # a dark tile, levels 50..114: the gain is 2 to 3
    return {"random": synth.noise_u8((2, 3, 33, 47), 16), "dark": dark, "real": real[:3, :, 300:450, 400:603].contiguous(), "he": torch.cat([synth.he_tile(32, 36, seed) for seed in (63, 65, 70)])}      # (tiles of whole packs; seeds whose median L* is above 30)


@pytest.fixture(scope="module")
def restated(dev, real_u8):
    """(tag, name, percentile) -> (GPU output on the CPU, restatement): the reference is computed once and shared."""
    cache = {}

    def get(tag: str, name: str, percentile: float):
        key = (tag, name, percentile)
        if key not in cache:
            x = synth.as_dtype(restatement_inputs(real_u8)[tag], TORCH_DTYPES[name]).to(dev)
            std = LuminosityStandardizer(percentile)
            est = std.estimate(x)
            out = std.apply(x, est)
            start = x.cpu().double().numpy() if name != "u8" else x.cpu().numpy()      # (f16 / bf16: the restatement starts from the rounded input)
            cache[key] = (out.cpu(), ln.standardize_unit(start, est.luminance.cpu().numpy()), est.lightness.cpu().numpy())
        return cache[key]

    return get


@pytest.mark.parametrize("percentile", [50.0, 95.0, 100.0])
@pytest.mark.parametrize("tag", ["random", "dark", "real", "he"])
@pytest.mark.parametrize("name", DTYPES)
def test_apply_against_the_restatement(restated, name, tag, percentile):
    """float32, float64: 1e-4 on [0, 1].  uint8: at most 1 level, fewer than 5e-3 of the elements differ.  f16, bf16: at most 2^-8, fewer
    than 2e-2 differ (the restatement rounded to the type).  The gain 100 / L_p stays at or below about 3.3 (L_p >= 30)."""
    out, ref, l_p = restated(tag, name, percentile)
    assert l_p.min() >= 30.0, (tag, percentile, l_p)
    if name in ("f32", "f64"):
        diff = np.abs(out.double().numpy() - ref)
        print(f"{tag} {name} p{percentile}: max |diff| {diff.max():.3e}, L_p {l_p.min():.1f}..{l_p.max():.1f}")
        assert diff.max() <= 1e-4, (tag, name, percentile, diff.max())
    elif name == "u8":
        diff = np.abs(out.numpy().astype(np.int64) - ln.to_levels(ref).astype(np.int64))
        print(f"{tag} u8 p{percentile}: max {diff.max()} levels, share {np.mean(diff > 0):.3e}, L_p {l_p.min():.1f}..{l_p.max():.1f}")
        assert diff.max() <= 1 and np.mean(diff > 0) < 5e-3, (tag, percentile, diff.max(), np.mean(diff > 0))
    else:
        want = torch.from_numpy(ref).to(TORCH_DTYPES[name]).double().numpy()
        diff = np.abs(out.double().numpy() - want)
        print(f"{tag} {name} p{percentile}: max |diff| {diff.max():.3e}, share {np.mean(diff > 0):.3e}, L_p {l_p.min():.1f}..{l_p.max():.1f}")
        assert diff.max() <= 2.0 ** -8 and np.mean(diff > 0) < 2e-2, (tag, name, percentile, diff.max(), np.mean(diff > 0))
