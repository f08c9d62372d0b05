#!/usr/bin/env python3
"""Three-stain colour deconvolution with a given basis: separate a batch into its stains, edit one and rebuild the tiles, jitter the
concentrations for training ("HED-light"), feed a slide's ESTIMATED H&E basis, complemented, through the same lossless path, and
measure a slide (positive-pixel fraction, H-score, percentiles) from integer histograms without writing a concentration map.
Run on a ROCm GPU:  python examples/deconvolve_stains.py"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stainx_amd import ColorDeconvolution, HEDAugment, Macenko, StainHistograms, stain_basis, synth  # noqa: E402


def main() -> None:
    dev = torch.device("cuda", 0)
    tiles = synth.he_batch(8, 256, 256, seed0=2024).to(dev)          # uint8 (N,3,H,W)

    # 1. a fixed basis: "hed" (haematoxylin, eosin, DAB), "he" or "hdab" (two stains and their complement), or your own (3, 3) matrix
    print("hed basis, columns are stain vectors:\n", stain_basis("hed"))
    cd = ColorDeconvolution("hed", device=dev)
    sep = cd.separate(tiles, stains=True, concentrations=True)       # one launch: three images per tile and three concentration maps
    print("stain images", tuple(sep.images.shape), sep.images.dtype, " concentrations", tuple(sep.concentrations.shape))

    # 2. lossless: edit a concentration, rebuild the tile (two launches) -- or do the same in one launch with per-tile factors
    conc = sep.concentrations.clone()
    conc[:, 1] *= 0.5                                                # half the eosin
    paler = cd.combine(conc)                                         # uint8 again
    n = tiles.shape[0]
    alpha = torch.tensor([[1.0, 0.5, 1.0]] * n, device=dev)
    same = cd.apply(tiles, alpha, torch.zeros(n, 3, device=dev))
    print("combine(edited) vs apply(alpha): max difference", int((paler.int() - same.int()).abs().max()), "grey level(s)")

    # 3. training-time jitter with the fixed basis: no estimate, one streaming launch, works on any stain and on near-empty tiles
    aug = HEDAugment(0.05, 0.05, mask="luminosity", generator=torch.Generator().manual_seed(0))
    out = aug(tiles)                                                 # float32 in [0, 1]; glass is copied, only tissue is jittered
    print("HEDAugment", tuple(out.shape), out.dtype, f"mean {out.mean().item():.3f}")

    # 4. an estimated H&E basis, complemented: the part of the optical density outside the H&E plane becomes a channel of its own
    est = Macenko(device=dev).estimate(tiles, pooled=True)           # one basis for the batch (a slide)
    own = ColorDeconvolution(est.complement(), device=dev)
    residual = own.separate(tiles, stains=False, concentrations=True).concentrations[:, 2]
    print(f"residual concentration outside the estimated H&E plane: mean |C_3| = {residual.abs().mean().item():.4f}")

    # 5. measure instead of map: one streaming launch per batch gives 256-bin integer histograms of the three concentrations (bins of 1/32
    # over [-2, 6) by default), their exact sums and the counted pixels -- no (N, 3, H, W) map is written.  Integer counts add up exactly:
    # pool the batches of a slide, then read the figures off the pooled set.  Thresholds are bin edges, so the figures are exact.
    ihc = ColorDeconvolution("hdab", device=dev, mask="luminosity")  # stain 1 is DAB; only tissue pixels count
    slide = StainHistograms.pool(*[ihc.quantify(batch, pooled=True) for batch in tiles.split(4)])
    print(f"tissue pixels {int(slide.pixels[0])}, mean DAB concentration {slide.mean()[0, 1].item():.4f}, "
          f"DAB-positive fraction (C >= 0.25) {slide.positive_fraction(1, 0.25)[0].item():.4f}, "
          f"H-score {slide.h_score(1, (0.25, 0.5, 1.0))[0].item():.1f}, 95th percentile bin {slide.quantile(1, 0.95)[0].item():.5f}")


if __name__ == "__main__":
    main()
