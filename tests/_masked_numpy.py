"""The yardstick of the tissue-mask tests: masked Reinhard and histogram matching restated in numpy from the CPU oracle's own functions
(oracle/stain_oracle.py, imported and unchanged) -- statistics in float64 over the masked pixels, ``hm_lut(bincount over the mask, ref,
n_tissue)``, background pixels copied.  With an all-ones mask every function returns exactly what the oracle's unmasked one returns
(tests/test_tissue_mask_cpu.py pins that).  Also the seeded inputs with background that both test files use."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import stain_oracle as so
from stainx_amd import synth

F32 = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
L_CUT = 204.0      # luminosity_threshold 0.8 on the oracle's 0..255 L scale (L* x 2.55)
L_BAND = 2e-2      # pixels whose oracle L is nearer to the cut are left out of rule comparisons (ten times the 2e-3 LAB units allowed a mean)
BORDER_CAP = 1e-3  # ... and may be at most this share of a case


# ------------------------------------------------------------------ the rule
def lightness(images: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """(N, H, W) float32: the oracle's L (0..255) of every pixel."""
    chw, _ = so._channels_first(images, channel_axis)
    return so.rgb_to_lab(so.to_unit_float(np.ascontiguousarray(chw)))[:, 0]


def rule_mask(images: np.ndarray, threshold: float = 0.8, channel_axis: int = 1) -> tuple[np.ndarray, np.ndarray]:
    """(tissue (N, H, W) bool, decided (N, H, W) bool): L < 255 * threshold, and where L is further than L_BAND from the cut."""
    lum = lightness(images, channel_axis)
    cut = 255.0 * threshold
    return lum < F32(cut), np.abs(lum.astype(np.float64) - cut) > L_BAND


# ------------------------------------------------------------------ Reinhard
def masked_mean_std(lab: np.ndarray, mask: np.ndarray) -> tuple[np.ndarray, np.ndarray, int]:
    """so._pooled_mean_std over the pixels of ``mask`` ((N, H, W) bool); fewer than two of them: NaN, NaN."""
    flat = np.transpose(lab, (1, 0, 2, 3)).reshape(3, -1)[:, mask.reshape(-1)].astype(np.float64)
    n = flat.shape[1]
    if n < 2:
        return np.full(3, np.nan, F32), np.full(3, np.nan, F32), n
    return flat.mean(axis=1).astype(F32), flat.std(axis=1, ddof=1).astype(F32), n


def reinhard_stats(images: np.ndarray, mask: np.ndarray, per_tile: bool):
    """(mean (rows, 3), std (rows, 3), counts (rows,)) over the tissue: every tile its own row, or one pooled row."""
    lab = so.rgb_to_lab(so.to_unit_float(images))
    groups = [slice(i, i + 1) for i in range(images.shape[0])] if per_tile else [slice(None)]
    rows = [masked_mean_std(lab[g], mask[g]) for g in groups]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int64)


def reinhard_fit(images: np.ndarray, mask: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    mean, std, _ = reinhard_stats(images, mask, per_tile=False)
    return mean[0], std[0]


def reinhard_apply(images: np.ndarray, mean: np.ndarray, std: np.ndarray, ref_mean, ref_std, mask: np.ndarray) -> np.ndarray:
    """so.reinhard_transform's arithmetic with GIVEN source statistics ((1, 3) or (N, 3)) on the tissue; background and NaN rows copied."""
    out = images.copy()
    rm = np.asarray(ref_mean, dtype=F32).reshape(1, 3, 1, 1)
    rs = np.asarray(ref_std, dtype=F32).reshape(1, 3, 1, 1)
    for i in range(images.shape[0]):
        m, s = (mean[i], std[i]) if mean.shape[0] > 1 else (mean[0], std[0])
        if np.isnan(m).any() or np.isnan(s).any():
            continue
        lab = so.rgb_to_lab(so.to_unit_float(images[i:i + 1]))
        lab_n = ((lab - m.astype(F32).reshape(1, 3, 1, 1)) / (s.astype(F32).reshape(1, 3, 1, 1) + F32(1e-8))) * rs + rm
        rgb = np.clip(so.lab_to_rgb(lab_n.astype(F32)), F32(0), F32(1))
        res = so.restore_dtype(rgb, images.dtype, in_0_255=False)
        out[i] = np.where(mask[i][None], res[0], images[i])
    return out


def reinhard_transform(images: np.ndarray, ref_mean, ref_std, mask: np.ndarray, per_tile: bool) -> np.ndarray:
    mean, std, _ = reinhard_stats(images, mask, per_tile)
    return reinhard_apply(images, mean, std, ref_mean, ref_std, mask)


# ------------------------------------------------------------------ histogram matching
def hm_counts(images: np.ndarray, mask: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """(3, 256) int64: the grey-level histograms of the masked pixels of the whole batch."""
    chw, _ = so._channels_first(images, channel_axis)
    u8, _ = so.images_to_uint8(chw)
    return np.stack([np.bincount(u8[:, c][mask], minlength=256) for c in range(3)]).astype(np.int64)


def hm_fit(images: np.ndarray, mask: np.ndarray, channel_axis: int = 1) -> list[np.ndarray]:
    hists = []
    for counts in hm_counts(images, mask, channel_axis):
        counts = counts.astype(F32)
        hists.append(counts / (so._torch_sum_f32(counts) + F32(1e-8)))
    return hists


def hm_transform(images: np.ndarray, ref_hists, mask: np.ndarray, per_tile: bool, channel_axis: int = 1, *, return_tables: bool = False):
    """so.hm_transform with ``hm_lut(counts over the mask, ref, n_tissue)`` per tile or pooled; background pixels are the input's."""
    chw, permuted = so._channels_first(images, channel_axis)
    dtype = chw.dtype
    u8, scaled_back = so.images_to_uint8(chw)
    n_img = u8.shape[0]
    groups = [slice(i, i + 1) for i in range(n_img)] if per_tile else [slice(None)]
    out = np.zeros(u8.shape, dtype=F32)
    tables = {"counts": [], "lut": [], "tissue": []}
    for g in groups:
        n_tissue = int(mask[g].sum())
        counts = hm_counts(np.ascontiguousarray(chw[g]), mask[g], 1)
        luts = [so.hm_lut(counts[c], np.asarray(ref_hists[min(c, len(ref_hists) - 1)]), n_tissue) for c in range(3)]
        for c in range(3):
            out[g, c] = luts[c][u8[g, c]]
        tables["counts"].append(counts)
        tables["lut"].append(np.stack(luts))
        tables["tissue"].append(n_tissue)
    if scaled_back:
        result = so.restore_dtype(np.clip(out / F32(255.0), F32(0), F32(1)), dtype, in_0_255=False)
    else:
        result = so.restore_dtype(np.clip(out, F32(0), F32(255)), dtype, in_0_255=True)
    result = np.where(mask[:, None], result, chw)
    if permuted:
        result = np.transpose(result, (0, 2, 3, 1))
    result = np.ascontiguousarray(result)
    if return_tables:
        return result, {"counts": np.stack(tables["counts"]), "lut": np.stack(tables["lut"]), "tissue": np.array(tables["tissue"], dtype=np.int64)}
    return result


# ------------------------------------------------------------------ inputs (seeded, all with background)
def striped_tiles() -> torch.Tensor:
    """(a): six Beer-Lambert tiles with glass stripes: tissue shares 1.0, 0.8, 0.6, 0.4, 0.2, 0.0 under the rule."""
    return synth.background_stripes(synth.he_batch(6, 96, 96, seed0=500, scale_step=0.1))


def noise_tiles(shape=(5, 3, 200, 328), seed: int = 7) -> torch.Tensor:
    """(b): uniform noise, tissue share 0.83-0.84 under the rule."""
    return synth.noise_u8(shape, seed)


def real_images() -> tuple[torch.Tensor, list[str]]:
    data = np.load(GOLDEN / "g11_real_images.npz")
    return torch.from_numpy(data["images_u8"]), [str(n) for n in data["names"]]


def real_crops(size: int = 512) -> torch.Tensor:
    """(c): the top-left crops of the real-tissue fixture (``test_5``: a tenth tissue)."""
    images, _ = real_images()
    return images[:, :, :size, :size].contiguous()


def oracle_input(x: torch.Tensor) -> np.ndarray:
    return x.numpy() if x.dtype in (torch.uint8, torch.float32) else x.float().numpy()      # (bf16 / f16 -> float32 is exact)


def oracle_cast(arr: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dtype)
