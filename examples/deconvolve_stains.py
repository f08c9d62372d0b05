#!/usr/bin/env python3
"""Three-stain colour deconvolution with a given basis: separate a batch into its stains, edit one and rebuild the tiles, jitter the
concentrations for training ("HED-light"), and feed a slide's ESTIMATED H&E basis, complemented, through the same lossless path.
Run on a ROCm GPU:  python examples/deconvolve_stains.py"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from stainx_amd import ColorDeconvolution, HEDAugment, Macenko, stain_basis, synth  # noqa: E402


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


if __name__ == "__main__":
    main()
