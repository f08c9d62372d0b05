"""The yardstick of the slide-level histogram-matching tests, restated in numpy from the CPU oracle's own functions (oracle/stain_oracle.py,
imported and unchanged): per-tile and pooled bincounts, tables by ``hm_lut`` row by row, and the lookup with GIVEN tables in the
reference's order of operations (``so.hm_transform``: gather, then / 255 and clamp for floats, then the dtype)."""
from __future__ import annotations

import numpy as np

from oracle import stain_oracle as so

F32 = np.float32


def bincounts(images: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """(N, 3, 256) int64: the grey-level histogram of every tile and channel (sum over axis 0: the pooled one)."""
    chw, _ = so._channels_first(images, channel_axis)
    u8, _ = so.images_to_uint8(np.ascontiguousarray(chw))
    return np.stack([np.stack([np.bincount(u8[t, c].reshape(-1), minlength=256) for c in range(3)]) for t in range(u8.shape[0])]).astype(np.int64)


def tables(counts: np.ndarray, pixels: np.ndarray, ref_hists) -> np.ndarray:
    """(S, 3, 256) float32: ``so.hm_lut`` of every row; a set without pixels gets the identity table (the documented divergence)."""
    out = np.empty(counts.shape, dtype=F32)
    for s in range(counts.shape[0]):
        for c in range(3):
            out[s, c] = np.arange(256, dtype=F32) if int(pixels[s]) == 0 else so.hm_lut(counts[s, c], np.asarray(ref_hists[c]), int(pixels[s]))
    return out


def lookup(images: np.ndarray, luts: np.ndarray, channel_axis: int = 1) -> np.ndarray:
    """``so.hm_transform`` from its gather on, with GIVEN tables ``luts`` (1, 3, 256) or (N, 3, 256): tile t takes row t (or row 0).
    A table entry outside 0..255 is clamped before the cast of EVERY output type, uint8 included, and a NaN entry is 0 (the library's
    rule, include/stainx_hip.h: sx_hm_apply_tables; the reference builds its own tables and never meets such an entry); an entry of
    -0.0 comes out as +0.0, as the device's max(v, 0) returns it (numpy's clip would keep the sign)."""
    luts = np.where(np.isnan(luts) | (luts == 0), F32(0), luts).astype(F32)
    chw, permuted = so._channels_first(images, channel_axis)
    dtype = chw.dtype
    u8, scaled_back = so.images_to_uint8(np.ascontiguousarray(chw))
    out = np.empty(u8.shape, dtype=F32)
    for t in range(u8.shape[0]):
        for c in range(3):
            out[t, c] = luts[t if luts.shape[0] > 1 else 0, c][u8[t, c]]
    if scaled_back:
        result = so.restore_dtype(np.clip(out / F32(255.0), F32(0), F32(1)), dtype, in_0_255=False)
    else:
        result = so.restore_dtype(np.clip(out, F32(0), F32(255)), dtype, in_0_255=True)
    if permuted:
        result = np.transpose(result, (0, 2, 3, 1))
    return np.ascontiguousarray(result)
