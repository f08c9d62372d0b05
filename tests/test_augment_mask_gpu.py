"""Stain augmentation under tissue masks and with a given source basis on the GPU (include/stainx_hip.h: sx_macenko_augment_masked;
MacenkoAugment(mask=..., source=...)).

* bit for bit: an all-ones mask = augment; augment_masked = estimate_masked + apply_masked with the factors, in both modes;
  alpha = 1, beta = 0 in normalise mode = transform_masked; masked-out pixels and tiles without an estimate are the background rule's
  copy; values under the mask do not matter;
* a captured call is one chain and replays on new images, mask bytes and factors; a poisoned workspace changes nothing;
* the C ABI's argument errors enqueue nothing; the module's mask and source options.
"""
from __future__ import annotations

import pytest
import torch

from oracle import stain_oracle as so
from stainx_amd import Macenko, MacenkoAugment, _native, synth, tissue_mask
from tests import _macenko_masked_numpy as mm
from tests import _masked_numpy as mn
from tests.conftest import TORCH_DTYPES
from tests.test_macenko_mask_gpu import background_expected, inside, mask_t, same_bits, unaligned_copy

pytestmark = pytest.mark.gpu

CLASSIC = _native.MACENKO_CLASSIC


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be(dev):
    from stainx_amd.backends.torch_hip_backend import MacenkoHIP

    return MacenkoHIP(dev)


@pytest.fixture(scope="module")
def ref(dev):
    he, mc = so.macenko_fit(synth.reference_tile(64, 64).numpy())
    return torch.from_numpy(he).to(dev), torch.from_numpy(mc).to(dev)


@pytest.fixture(scope="module")
def real():
    x = mn.real_crops(256)
    return x, mn.rule_mask(x.numpy())[0]


def shapes(real_tiles: torch.Tensor):
    yield "64x64", synth.he_batch(3, 64, 64)
    yield "33x47", synth.he_batch(2, 33, 47)
    yield "30x30", synth.he_batch(3, 30, 30)
    yield "5x4", synth.he_batch(1, 40, 32)[:, :, 4::8, 4::8].contiguous()
    yield "96x96", synth.he_batch(2, 96, 96, seed0=77)      # (several work items of the wider packs; the real crops, 65536 pixels, are four items of the uint8 pack's 16384)
    yield "real", real_tiles


def masks_for(tiles: torch.Tensor):
    n, _, h, w = tiles.shape
    yield "disc", mm.disc(n, h, w)
    yield "blocks16", mm.blocks(n, h, w, 16)
    yield "blocks5", mm.blocks(n, h, w, 5)
    yield "rule", mn.rule_mask(tiles.numpy())[0]
    yield "two", mm.exactly(n, h, w, 2)
    yield "three", mm.exactly(n, h, w, 3)
    yield "zeros", mm.zeros(n, h, w)


def factors(n: int, dev, seed: int = 11) -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.3 * (2.0 * torch.rand(n, 2, generator=g) - 1.0)).to(dev), (0.2 * (2.0 * torch.rand(n, 2, generator=g) - 1.0)).to(dev)


def options_for(dt: torch.dtype):
    yield {}
    yield {"normalize_to_0_1": True}
    if dt == torch.uint8:
        yield {"out_dtype": torch.bfloat16}
        yield {"out_dtype": torch.float16, "normalize_to_0_1": True}


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view(torch.uint8).view(t.shape + (-1,))


# ------------------------------------------------------------------------------------------------ 1. the identities, bit for bit
@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_all_ones_mask_is_augment(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    for what, tiles in shapes(real[0]):
        x = synth.as_dtype(tiles, dt).to(dev)
        n, _, h, w = x.shape
        m = torch.ones((n, h, w), dtype=torch.uint8, device=dev)
        alpha, beta = factors(n, dev)
        for reference in ((None, None), ref):
            for opt in options_for(dt):
                assert same_bits(be.augment_masked(x, alpha, beta, *reference, m, **opt), be.augment(x, alpha, beta, *reference, **opt)), (what, reference[0] is None, opt)


@pytest.mark.parametrize("name", list(TORCH_DTYPES))
def test_masked_identities_and_background(dev, be, ref, real, name):
    dt = TORCH_DTYPES[name]
    for what, tiles in shapes(real[0]):
        x = synth.as_dtype(tiles, dt).to(dev)
        n = x.shape[0]
        alpha, beta = factors(n, dev)
        ones, zeros = torch.ones(n, 2, device=dev), torch.zeros(n, 2, device=dev)
        for mask_name, mask in masks_for(tiles):
            m = mask_t(mask, dev)
            est = be.estimate_masked(x, m)
            where = torch.from_numpy(inside(mask, x).copy())
            has = torch.isfinite(est["he"]).all(dim=2).all(dim=1).cpu()
            if mask_name in ("two", "zeros"):
                assert not bool(has.any()), (what, mask_name)
            copied = ~where | ~has.view(n, 1, 1, 1)      # masked-out pixels, and every pixel of a tile without an estimate
            for reference in ((None, None), ref):
                for opt in options_for(dt):
                    tag = (what, mask_name, reference[0] is None, opt)
                    got = be.augment_masked(x, alpha, beta, *reference, m, **opt)
                    # augment_masked = estimate_masked + apply_masked with the factors
                    assert same_bits(got, be.apply_masked(x, est["he"], est["max_c"], *reference, m, alpha=alpha, beta=beta, **opt)), tag
                    # the background: exactly the background rule, / 255 and uint8 -> bf16 / f16 included
                    want = background_expected(x.cpu(), opt.get("normalize_to_0_1", False), opt.get("out_dtype"))
                    assert got.dtype == want.dtype and torch.equal(bits(got.cpu())[copied], bits(want)[copied]), tag
                    # alpha = 1, beta = 0 in normalise mode: the masked transform
                    if reference[0] is not None:
                        assert same_bits(be.augment_masked(x, ones, zeros, *reference, m, **opt), be.transform_masked(x, *reference, m, **opt)), tag
            # values under the mask do not matter
            if dt != torch.uint8:
                want = be.augment_masked(x, alpha, beta, *ref, m).cpu()
                for fill in (float("nan"), float("inf"), float("-inf")):
                    y = torch.where(where.to(dev), x, torch.full_like(x, fill))
                    again = be.augment_masked(y, alpha, beta, *ref, m).cpu()
                    assert torch.equal(bits(again)[where], bits(want)[where]), (what, mask_name, fill)
        # images and mask one element off a 16-byte address, independently: the scalar path, the same bits
        m = mask_t(mm.blocks(n, x.shape[2], x.shape[3], 5), dev)
        want = be.augment_masked(x, alpha, beta, *ref, m)
        for xa, ma in ((unaligned_copy(x), m), (x, unaligned_copy(m)), (unaligned_copy(x), unaligned_copy(m))):
            assert same_bits(be.augment_masked(xa, alpha, beta, *ref, ma), want), what


def test_a_nan_source_row_copies_the_tile_and_neighbours_are_untouched(dev, be, ref, real):
    x8 = torch.cat([real[0][[5, 3]], synth.background_stripes(synth.he_batch(3, 256, 256))[1:]])      # glass crop, tissue crop, half glass, all glass
    x = synth.as_dtype(x8, torch.float32).to(dev)
    alpha, beta = factors(4, dev)
    made, counts = tissue_mask(x, 0.8)
    empty = (counts < 3).cpu()
    assert bool(empty[0]) and bool(empty[3]) and not bool(empty[1]) and not bool(empty[2])
    bg = background_expected(x.cpu(), True)
    for reference in ((None, None), ref):
        out = be.augment_masked(x, alpha, beta, *reference, made, normalize_to_0_1=True).cpu()
        assert same_bits(out[empty], bg[empty]) and not torch.isnan(out).any()
        one = be.augment_masked(x[1:2].contiguous(), alpha[1:2].contiguous(), beta[1:2].contiguous(), *reference, made[1:2].contiguous(), normalize_to_0_1=True).cpu()
        assert same_bits(one, out[1:2])
        # the module with a given source whose rows hold NaN for the tiles without tissue: those tiles are copied whatever the mask says
        est = be.estimate_masked(x, made)
        norm = None
        if reference[0] is not None:
            norm = Macenko(device=dev)
            norm._stain_matrix, norm._target_max_conc, norm._is_fitted = reference[0], reference[1], True
        module = MacenkoAugment(0.3, 0.2, normalizer=norm, device=dev, source=(est["he"], est["max_c"]), mask="luminosity")
        all_in = torch.ones_like(made)
        got = module(x, alpha, beta, mask=all_in).cpu()
        assert same_bits(got[empty], bg[empty])
        assert same_bits(got, be.apply_masked(x, est["he"], est["max_c"], *reference, all_in, alpha=alpha, beta=beta, normalize_to_0_1=True).cpu())


# ------------------------------------------------------------------------------------------------ 2. plumbing
def test_poisoned_workspace_side_stream_and_graph(dev, be, ref, real):
    sm, tmc = ref
    x8, rule = real
    x = synth.as_dtype(x8[:4], torch.float32).to(dev)
    x2 = synth.as_dtype(x8[[3, 2, 1, 0]], torch.float32).to(dev)
    m, m2 = mask_t(rule[:4], dev), mask_t(mm.blocks(4, 256, 256, 16, seed=8), dev)
    (alpha, beta), (alpha2, beta2) = factors(4, dev), factors(4, dev, seed=12)
    for reference in ((None, None), (sm, tmc)):
        want, want2 = be.augment_masked(x, alpha, beta, *reference, m), be.augment_masked(x2, alpha2, beta2, *reference, m2)
        assert not same_bits(want, want2)
        for fill in (0xFF, 0x7F):      # a workspace poisoned beforehand changes nothing
            be.last_workspace.fill_(fill)
            assert same_bits(be.augment_masked(x, alpha, beta, *reference, m), want), fill
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            on_side = be.augment_masked(x, alpha, beta, *reference, m)
        side.synchronize()
        assert same_bits(on_side, want)
        # a captured call: one chain on one stream, replayed after new images, mask bytes and factors were copied into the same buffers
        xbuf, mbuf, abuf, bbuf = x.clone(), m.clone(), alpha.clone(), beta.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            be.augment_masked(xbuf, abuf, bbuf, *reference, mbuf)      # (warm-up on the capture stream: its workspace exists before the capture)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                captured = be.augment_masked(xbuf, abuf, bbuf, *reference, mbuf)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(captured, want)
        xbuf.copy_(x2)
        mbuf.copy_(m2)
        abuf.copy_(alpha2)
        bbuf.copy_(beta2)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(captured, want2)


def test_c_abi_argument_errors_enqueue_nothing_and_a_raw_call_works(dev, be, ref):
    lib = _native.require()
    sm, tmc = ref
    x = synth.as_dtype(synth.he_batch(2, 64, 64), torch.float32).to(dev)
    m = torch.ones(2, 64, 64, dtype=torch.uint8, device=dev)
    out = torch.full_like(x, -7.0)
    alpha, beta = factors(2, dev)
    code = _native.DTYPE_CODES[torch.float32]
    ws = torch.empty(int(lib.sx_macenko_workspace_bytes_for(code, 2, 64, 64, CLASSIC)), dtype=torch.uint8, device=dev)
    stream = _native.stream_ptr(dev)
    BAD = _native.SX_ERR_BAD_ARG

    def call(o=out.data_ptr(), mask=m.data_ptr(), a=alpha.data_ptr(), b=beta.data_ptr(), s=sm.data_ptr(), t=tmc.data_ptr(), flags=0, nbytes=ws.numel()):
        return lib.sx_macenko_augment_masked(x.data_ptr(), o, code, 2, 64, 64, mask, a, b, s, t, flags, ws.data_ptr(), nbytes, stream)

    assert call(mask=None) == BAD and _native.last_error(lib)
    assert call(flags=_native.MACENKO_CHANNELS_LAST) == BAD and call(flags=_native.MACENKO_SAMPLED) == BAD
    assert call(o=None) == BAD and call(a=None) == BAD and call(b=None) == BAD
    assert call(s=None) == BAD and call(t=None) == BAD      # one of the reference pair
    assert call(nbytes=ws.numel() - 1) == _native.SX_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert call(flags=CLASSIC) == _native.SX_OK, _native.last_error(lib)
    assert same_bits(out, be.augment(x, alpha, beta, sm, tmc))
    assert call(s=None, t=None) == _native.SX_OK and same_bits(out, be.augment(x, alpha, beta))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the module
def test_module_mask_and_source(dev, be, ref, real):
    sm, tmc = ref
    x = real[0][:5].to(dev)
    made = tissue_mask(x, 0.8)[0]
    where = (made != 0)[:, None].expand(5, 3, 256, 256).cpu()
    bg = background_expected(x.cpu(), True)
    norm = Macenko(device=dev)
    norm._stain_matrix, norm._target_max_conc, norm._is_fitted = sm, tmc, True
    for normalizer in (None, norm):
        reference = (None, None) if normalizer is None else (sm, tmc)
        module = MacenkoAugment(0.3, 0.2, normalizer=normalizer, device=dev, mask="luminosity", generator=torch.Generator().manual_seed(5))
        out = module(x).cpu()
        # every masked-out pixel is the background rule's copy; masked-in pixels change with sigma > 0
        assert out.dtype == bg.dtype and torch.equal(bits(out)[~where], bits(bg)[~where])
        still = MacenkoAugment(0.0, 0.0, normalizer=normalizer, device=dev, mask="luminosity")(x).cpu()
        assert torch.equal(bits(still)[~where], bits(bg)[~where])
        assert (out[where] != still[where]).float().mean().item() > 0.5
        # explicit factors: the backend call; an explicit mask for the call wins over the rule
        alpha, beta = factors(5, dev)
        assert same_bits(module(x, alpha, beta), be.augment_masked(x, alpha, beta, *reference, made, normalize_to_0_1=True))
        disc = mask_t(mm.disc(5, 256, 256), dev)
        assert same_bits(module(x, alpha, beta, mask=disc), be.augment_masked(x, alpha, beta, *reference, disc, normalize_to_0_1=True))
        plain = MacenkoAugment(0.3, 0.2, normalizer=normalizer, device=dev)
        assert same_bits(plain(x, alpha, beta, mask="luminosity"), module(x, alpha, beta)) and same_bits(plain(x, alpha, beta), be.augment(x, alpha, beta, *reference, normalize_to_0_1=True))
        # a given source: Macenko.apply with the module's drawn factors, one launch
        slide = Macenko(device=dev).estimate(x, pooled=True)
        seeded = MacenkoAugment(0.3, 0.2, normalizer=normalizer, device=dev, source=slide, generator=torch.Generator().manual_seed(9))
        drawn = MacenkoAugment(0.3, 0.2, generator=torch.Generator().manual_seed(9)).sample_factors(5, dev)
        unit = Macenko(device=dev, normalize_to_0_1=True)
        unit._stain_matrix, unit._target_max_conc, unit._is_fitted = sm, tmc, True
        want = unit.apply(x, slide, alpha=drawn[0], beta=drawn[1], own_basis=normalizer is None)
        assert same_bits(seeded(x), want)
        masked_source = MacenkoAugment(0.3, 0.2, normalizer=normalizer, device=dev, source=slide, mask="luminosity")
        assert same_bits(masked_source(x, alpha, beta), unit.apply(x, slide, alpha=alpha, beta=beta, own_basis=normalizer is None, mask="luminosity"))
        # a single CHW tile with its (H, W) mask
        assert same_bits(module(x[0], alpha[:1], beta[:1], mask=made[0]), module(x[:1], alpha[:1], beta[:1])[0])
