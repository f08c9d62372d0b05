#!/usr/bin/env python3
"""The hot path in five lines each: the three normalisers, the nn.Module, uint8 HWC tiles as a decoder hands them over,
the sampled `precision="fast"` mode, how a batch is split over GPUs (one process per GPU, no collective for
`transform`), the slide-level use: one source estimate, applied to batch after batch, per-tile statistics for Reinhard and
histogram matching on a batch of tiles from different slides, their tissue masks for tiles with slide background, and slide-level
histogram matching (histograms added up over batches, one table, one launch per batch), and a tissue mask detected on the device and
cleaned by area (small objects go, small holes are filled), and Vahadane's stain estimate behind the same surface, and a Macenko estimate on
tissue pixels sampled from several batches.  Run on a ROCm GPU:  python examples/normalize_tiles.py
Under torchrun (`python -m torch.distributed.run --nproc-per-node N examples/normalize_tiles.py`) every rank works on
its own slice of the batch and the last section pools a Macenko fit over all ranks."""
from __future__ import annotations

import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stainx_amd import (HistogramMatching, HistogramStatistics, Macenko, PixelSample, Reinhard, StainNormalizerTransform, mask_components, otsu_mask,  # noqa: E402
                        remove_small_holes, remove_small_objects, sample_pixels, synth, tissue_mask, Vahadane)
from stainx_amd import distributed as sxd  # noqa: E402
from stainx_amd.backends.torch_hip_backend import MacenkoHIP  # noqa: E402


def main() -> None:
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=dev)

    reference = synth.reference_tile(256, 256)                       # uint8 (1,3,H,W): the look every tile should get
    batch = synth.he_batch(16, 256, 256, seed0=2024)                 # uint8 (N,3,H,W) synthetic H&E tiles
    lo, hi = sxd.shard_bounds(batch.shape[0], rank, world)           # this rank's tiles: transform needs no communication
    tiles = batch[lo:hi].to(dev)

    # 1. the three normalisers -- same constructor / fit / transform as `from stainx import ...`
    for cls in (Macenko, Reinhard, HistogramMatching):
        out = cls(device=dev).fit(reference.to(dev)).transform(tiles)
        print(f"[rank {rank}] {cls.__name__:18s} {tuple(out.shape)} {out.dtype}  mean {out.float().mean().item():.2f}")

    # 2. as an nn.Module in a preprocessing pipeline (float tiles in [0,1], output in [0,1])
    module = StainNormalizerTransform(method="macenko", mode="reference", reference=synth.as_dtype(reference, torch.bfloat16).to(dev))
    out = module(synth.as_dtype(batch[lo:hi], torch.bfloat16).to(dev))
    print(f"[rank {rank}] module (bf16)        {tuple(out.shape)} {out.dtype}  range [{out.float().min().item():.3f}, {out.float().max().item():.3f}]")

    # 3. uint8 HWC tiles straight from a decoder: no permute / copy / float conversion before the call
    backend = MacenkoHIP(dev)
    he, max_c = backend.compute_reference_stain_matrix(reference.to(dev))
    hwc = tiles.permute(0, 2, 3, 1).contiguous()
    out = backend.transform(hwc, he, max_c, channels_last=True)
    # ... and straight to a model's input type: uint8 HWC in, bf16 in [0, 1] out, one call (== the line above / 255, .to(bfloat16))
    model_in = backend.transform(hwc, he, max_c, channels_last=True, normalize_to_0_1=True, out_dtype=torch.bfloat16)
    assert model_in.dtype == torch.bfloat16 and model_in.shape == hwc.shape
    print(f"[rank {rank}] uint8 NHWC          {tuple(out.shape)} {out.dtype}")

    # 4. sampled percentiles: about twice as fast, mean abs error ~0.5 grey levels against the exact transform
    exact = Macenko(device=dev).fit(reference.to(dev)).transform(tiles)
    fast = Macenko(device=dev, precision="fast").fit(reference.to(dev)).transform(tiles)
    print(f"[rank {rank}] precision='fast'    mean |fast - exact| = {(fast.float() - exact.float()).abs().mean().item():.3f} grey levels")

    # 5. one stain estimate pooled over the tiles of ALL ranks (a few small collectives), identical bits on every rank
    he_pooled, max_c_pooled = sxd.macenko_fit_pooled(tiles)
    print(f"[rank {rank}] pooled fit          HE[:,0] = {[round(v, 4) for v in he_pooled[:, 0].tolist()]}  maxC = {[round(v, 4) for v in max_c_pooled.tolist()]}")

    # 6. slide level: ONE source estimate for the slide (pooled over a batch of its tissue tiles), applied to that batch and to the next
    #    one -- neighbouring tiles get the same mapping, and a call is one launch: a pixel read, a pixel written, no estimate
    norm = Macenko(device=dev).fit(reference.to(dev))
    slide = norm.estimate(tiles, pooled=True)                        # StainEstimate: (1, 3, 2) stain vectors, (1, 2) maxC
    out = norm.apply(tiles, slide)
    more = synth.he_batch(8, 256, 256, seed0=4048).to(dev)           # more tiles of the same slide: no new estimate
    out_more = norm.apply(more, slide)
    tissue = Macenko(device=dev, mask="luminosity").fit(reference.to(dev))      # the estimate over tissue pixels only (edge tiles, thumbnails): glass is copied
    out_tissue = tissue.apply(tiles, tissue.estimate(tiles, pooled=True))       # ... also slide-level: one masked estimate, applied under the same rule
    per_tile = norm.estimate(tiles)                                  # every tile's own estimate fed back: the transform, bit for bit
    assert torch.equal(norm.apply(tiles, per_tile), norm.transform(tiles))
    sep = norm.separate(more, source=slide, concentrations=True)     # the slide's basis for separation too: one launch, H / E maps that line up across tiles
    sep_tissue = tissue.separate(tiles, concentrations=True)         # under the rule, glass holds no stain: concentrations 0, both images at the 240 level
    assert torch.equal(norm.separate(tiles, source=per_tile).hematoxylin, norm.separate(tiles).hematoxylin)
    assert sep.concentrations.shape == (8, 2, 256, 256) and sep_tissue.eosin.shape == tiles.shape
    print(f"[rank {rank}] slide-level apply   {tuple(out.shape)} + {tuple(out_more.shape)} {out.dtype}  maxC = {[round(v, 4) for v in slide.max_concentrations[0].tolist()]}")

    # 7. a batch of tiles from DIFFERENT slides (a DataLoader batch): Reinhard and histogram matching with every tile's own statistics --
    #    still two / three launches for the batch, and a tile's result does not depend on what else is in the batch
    mixed = torch.cat([tiles[:4], synth.noise_u8((4, 3, 256, 256), 7).to(dev)])
    for cls in (Reinhard, HistogramMatching):
        per_tile_norm = cls(device=dev, statistics="tile").fit(reference.to(dev))
        out = per_tile_norm.transform(mixed)
        assert torch.equal(per_tile_norm.transform(mixed.flip(0).contiguous()).flip(0), out)      # the same tiles among other neighbours: the same bits
        print(f"[rank {rank}] {cls.__name__ + ' per tile':27s} {tuple(out.shape)} {out.dtype}  mean {out.float().mean().item():.2f}")
    #    ... and a slide normalised with ONE set of LAB statistics, estimated once: one launch per batch afterwards
    reinhard = Reinhard(device=dev).fit(reference.to(dev))
    slide_stats = reinhard.estimate(tiles, pooled=True)              # ColorStatistics: (1, 3) mean, (1, 3) std
    out = reinhard.apply(tiles, slide_stats)
    out_more = reinhard.apply(more, slide_stats)
    assert torch.equal(out, reinhard.transform(tiles))               # the pooled transform of that batch, bit for bit
    print(f"[rank {rank}] Reinhard slide-level    {tuple(out.shape)} + {tuple(out_more.shape)}  LAB mean = {[round(v, 2) for v in slide_stats.mean[0].tolist()]}")

    # 8. tiles with slide background (edge tiles, sparse tiles, thumbnails): statistics over the TISSUE only, the glass left as it is.
    #    mask="luminosity" applies the rule L* / 100 < 0.8 in every kernel; an explicit mask (a segmentation) replaces it for one call
    edge = synth.background_stripes(batch[:6]).to(dev)               # tile i: a stripe of glass i / 5 of its width
    mask, counts = tissue_mask(edge, luminosity_threshold=0.8)       # (N, H, W) uint8 and (N,) tissue pixels, on the device
    for cls in (Reinhard, HistogramMatching):
        masked = cls(device=dev, statistics="tile", mask="luminosity").fit(reference.to(dev))
        out = masked.transform(edge)
        glass = (mask == 0).unsqueeze(1).expand_as(edge)
        assert torch.equal(out[glass], edge[glass])                  # background: the bits of the input
        assert torch.equal(cls(device=dev, statistics="tile").fit(reference.to(dev)).transform(edge, mask=mask), out)      # the rule == its own mask
        print(f"[rank {rank}] {cls.__name__ + ' tissue only':27s} {tuple(out.shape)} {out.dtype}  tissue share per tile {[round(c / (256 * 256), 2) for c in counts.tolist()]}")

    # 9. slide-level histogram matching: a slide arrives in many batches.  Histograms are integer counts, so those of the batches ADD UP
    #    EXACTLY: estimate each batch with the rule, pool, build the lookup table ONCE, then every batch is one launch
    hm = HistogramMatching(device=dev, mask="luminosity").fit(reference.to(dev))
    slide_tiles = torch.cat([edge, tiles, more])
    batches = list(slide_tiles.split(8))
    slide_hist = HistogramStatistics.pool(*[hm.estimate(b, pooled=True) for b in batches])      # counts (1, 3, 256), pixels (1,): int64 on the device
    #    (under torchrun: torch.distributed.all_reduce(slide_hist.counts), all_reduce(slide_hist.pixels) pools them over the ranks as well)
    table = hm.lookup_tables(slide_hist)                             # (1, 3, 256) float32
    out = torch.cat([hm.apply(b, table) for b in batches])
    assert torch.equal(out, HistogramMatching(device=dev, statistics="batch", mask="luminosity").fit(reference.to(dev)).transform(slide_tiles))      # the slide as ONE batch, bit for bit
    print(f"[rank {rank}] HistogramMatching slide     {tuple(out.shape)} in {len(batches)} batches  tissue pixels {slide_hist.pixels.item()}")

    # 10. a mask DETECTED on the device and cleaned BY AREA: Otsu's threshold pooled over the batch, then objects below 64 pixels go (dust,
    #     pen specks) and holes below 256 pixels are filled (fat, lumina) -- what an opening and a closing cannot do without eating the
    #     tissue's boundary and bridging its fragments.  Nothing returns to the host but Otsu's 256 counts.  A "hole" is ANY component of
    #     the background, the glass at a tile's edge included: keep min_hole_area below a tile's glass, or threshold a thumbnail.
    det = otsu_mask(edge, pooled=True, min_object_area=64, min_hole_area=256)
    raw = otsu_mask(edge, pooled=True)
    assert torch.equal(det.mask, remove_small_holes(remove_small_objects(raw.mask, 64)[0], 256)[0])      # the single calls, in that order
    found = mask_components(det.mask)                                # MaskComponents: canonical labels, areas at the first pixels, counts
    largest = found.areas.flatten(1).max(dim=1).values               # e.g. the largest tissue object of every tile, without leaving the device
    out = Macenko(device=dev).fit(reference.to(dev)).transform(edge, mask=det.mask)
    print(f"[rank {rank}] detected tissue mask        {tuple(out.shape)}  objects per tile {found.counts.tolist()}  largest {largest.tolist()}  tissue pixels {det.counts.tolist()}")
    # 11. Vahadane's estimator (sparse NMF of the optical density) behind Macenko's surface: a fixed number of rounds, so the call is
    #     deterministic and never synchronises; the estimate runs over the luminosity mask by default and glass is copied through.
    #     Its StainEstimate goes wherever Macenko's goes; max_concentrations() completes a basis that was estimated elsewhere.
    vahadane = Vahadane(device=dev, regularizer=0.1, iterations=30).fit(reference.to(dev))
    out = vahadane.transform(edge)
    slide = vahadane.estimate(edge, pooled=True)                     # one basis for the batch: apply() is one launch per batch afterwards
    out_slide = vahadane.apply(edge, slide)
    max_c = vahadane.max_concentrations(edge, slide.stain_matrices, pooled=True)
    assert torch.equal(max_c, slide.max_concentrations)
    print(f"[rank {rank}] Vahadane                    {tuple(out.shape)} + {tuple(out_slide.shape)} {out.dtype}  H = {[round(v, 3) for v in slide.stain_matrices[0, :, 0].tolist()]}  "
          f"E = {[round(v, 3) for v in slide.stain_matrices[0, :, 1].tolist()]}")
    # 12. a slide-level MACENKO estimate over several batches.  Percentiles do not add up the way histograms do, so every batch gives a
    #     bounded sample of its REAL tissue pixels -- an exact integer stride over the masked-in pixels of the batch, copied bit for bit
    #     into a fixed-shape tile with a validity mask --, the samples are concatenated, and ONE pooled masked estimate reads them; then
    #     `apply` per batch.  The sampler never synchronises (here only Otsu's 256 counts return to the host), and a thumbnail's mixed
    #     edge pixels never enter the estimate.
    mk = Macenko(device=dev).fit(reference.to(dev))
    samples = [sample_pixels(b, (64, 64), mask=otsu_mask(b, pooled=True).mask, pooled=True) for b in batches]
    sample = PixelSample.cat(*samples)                               # pixels (batches, 3, 64, 64), valid (batches, 64, 64): a small batch with a mask
    slide = mk.estimate(sample.pixels, pooled=True, mask=sample.valid)
    out = torch.cat([mk.apply(b, slide) for b in batches])
    print(f"[rank {rank}] Macenko on sampled tissue   {tuple(out.shape)} in {len(batches)} batches  sampled {sample.taken.tolist()} of {sample.population.tolist()} tissue pixels  "
          f"maxC = {[round(v, 4) for v in slide.max_concentrations[0].tolist()]}")
    # 13. statistics-space augmentation (RandStainNA): fit the cohort's distribution of per-tile statistics ONCE -- in LAB from
    #     Reinhard.estimate, in HED from ColorDeconvolution.estimate (exact integer moments, no map) --, then every tile of a training batch
    #     is moved from its OWN statistics to a target drawn from it: estimate + one apply launch, nothing returns to the host.
    from stainx_amd import ColorDeconvolution, StatisticsAugment, StatisticsDistribution

    lab_cohort = StatisticsDistribution.fit(*[Reinhard(device=dev, mask="luminosity").estimate(b) for b in batches])      # rows of tiles without tissue are skipped
    hed_cohort = StatisticsDistribution.fit(*[ColorDeconvolution("hed", device=dev, mask="luminosity").estimate(b) for b in batches])
    lab_aug = StatisticsAugment(lab_cohort, "lab", kind="normal", p=0.8, mask="luminosity", generator=torch.Generator().manual_seed(rank))
    hed_aug = StatisticsAugment(hed_cohort, "hed", kind="laplace", mask="luminosity", generator=torch.Generator().manual_seed(rank))
    out_lab, out_hed = lab_aug(edge), hed_aug(edge)
    glass = (tissue_mask(edge)[0] == 0).unsqueeze(1).expand_as(edge)
    assert torch.equal(out_lab[glass], edge[glass])                  # LAB: glass keeps the bits of the input
    print(f"[rank {rank}] StatisticsAugment           {tuple(out_lab.shape)} {out_lab.dtype} (lab) + {tuple(out_hed.shape)} {out_hed.dtype} (hed)  "
          f"cohort L* mean {lab_cohort.mean_center[0].item():.1f} +- {lab_cohort.mean_spread[0].item():.1f}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
