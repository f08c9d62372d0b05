"""Tissue pixel sampling: a bounded, fixed-shape set of real tissue pixels for slide-level estimates (HistomicsTK's ``sample_pixels``, exact
and on the device; an extension: the reference has none).

The slide-level estimates that are not additive -- Macenko's percentiles, Vahadane's NMF, the luminosity percentile -- cannot be pooled
batch by batch.  :func:`sample_pixels` writes, for every tile or for the batch as a whole, a tile of at most K masked-in pixels and a
validity mask; samples of any number of batches concatenate (:meth:`PixelSample.cat`) into one small batch that
``estimate(s.pixels, pooled=True, mask=s.valid)`` of every normaliser reads once.

The rule (include/stainx_hip.h: sx_sample_pixels).  A group is a tile, or with ``pooled=True`` the whole batch.  Its population
is its masked-in pixels, ranked 0 .. n-1 in raster order (pooled: tile after tile).  K = h * w of ``size``; slot j is pixel j of the output
tile in raster order.  ``n <= K``: slot r holds rank r and the slots from n on are zero bytes with ``valid = 0``.  ``n > K``: slot j holds rank
``(j * n + o) // K`` with ``o = offset % n``.  A pixel is moved as the three values of its element type: nothing is converted.
"""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe, masks

MAX_SAMPLE_SIZE = 1 << 24      # include/stainx_hip.h: sample_size
MAX_GROUP_PIXELS = (1 << 31) - 1


class PixelSample(NamedTuple):
    """What :func:`sample_pixels` returns, all on the device.  ``pixels``: (G, 3, h, w) in the element type of the images, always planar;
    ``valid``: (G, h, w) uint8, 1 where a slot holds a pixel; ``taken``: (G,) int32, ``min(population, h * w)``; ``population``: (G,) int64, the
    group's masked-in pixels.  G: one row per tile, or 1 for a pooled sample.  ``pixels`` with ``mask=valid`` is a batch every masked
    ``estimate`` accepts."""

    pixels: torch.Tensor
    valid: torch.Tensor
    taken: torch.Tensor
    population: torch.Tensor

    @staticmethod
    def cat(*samples: "PixelSample") -> "PixelSample":
        """The samples' groups, one after another along the first axis (a torch concatenation where the tensors live).  The samples must
        have the same ``(h, w)``, element type and device."""
        if not samples:
            raise ValueError("cat needs at least one PixelSample")
        for item in samples:
            if not (isinstance(item, (tuple, list)) and len(item) == 4 and all(isinstance(t, torch.Tensor) for t in item)):
                raise ValueError("expected PixelSamples (pixels, valid, taken, population)")
            pixels, valid, taken, population = item
            groups = pixels.shape[0] if pixels.dim() == 4 else -1
            if pixels.dim() != 4 or pixels.shape[1] != 3 or tuple(valid.shape) != (groups, pixels.shape[2], pixels.shape[3]) or tuple(taken.shape) != (groups,) or \
                    tuple(population.shape) != (groups,):
                raise ValueError(f"not a PixelSample: shapes {tuple(pixels.shape)}, {tuple(valid.shape)}, {tuple(taken.shape)}, {tuple(population.shape)}")
        first = samples[0][0]
        for item in samples[1:]:
            pixels = item[0]
            if tuple(pixels.shape[2:]) != tuple(first.shape[2:]):
                raise ValueError(f"samples must have the same size, got {tuple(first.shape[2:])} and {tuple(pixels.shape[2:])}")
            if pixels.dtype != first.dtype:
                raise ValueError(f"samples must have the same element type, got {first.dtype} and {pixels.dtype}")
            if pixels.device != first.device:
                raise ValueError(f"samples must live on the same device, got {first.device} and {pixels.device}")
        return PixelSample(*(torch.cat([item[i] for item in samples], dim=0) for i in range(4)))


def _check_size(size: Any) -> tuple[int, int]:
    def whole(value: Any) -> bool:
        return isinstance(value, int) and not isinstance(value, bool) and value >= 1

    if whole(size):
        h, w = 1, size
    elif isinstance(size, (tuple, list)) and len(size) == 2 and whole(size[0]) and whole(size[1]):
        h, w = size
    else:
        raise ValueError(f"size must be a positive int k (a 1 x k sample) or a pair (h, w) of positive ints, got {size!r}")
    if h * w > MAX_SAMPLE_SIZE:
        raise ValueError(f"size must hold at most 2^24 pixels, got {h} x {w}")
    return h, w


def sample_pixels(images: torch.Tensor, size: Any, *, mask: Any = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD, pooled: bool = False,
                  offset: int = 0, channel_axis: int = 1) -> PixelSample:
    """A sample of at most ``h * w`` masked-in pixels of every tile, or with ``pooled=True`` ONE of the whole batch: :class:`PixelSample`.

    ``images``: NCHW (``channel_axis=-1``: NHWC) with C = 3, any supported element type; a CPU tensor is moved to the current GPU.  ``size``:
    ``(h, w)``, or an int ``k`` for ``(1, k)``; at most 2^24 pixels.  ``mask``: None (every pixel), ``"luminosity"`` (the rule at ``luminosity_threshold``, as
    :func:`stainx_amd.tissue_mask` decides it) or an explicit uint8 / bool ``(N, H, W)`` / ``(N, 1, H, W)`` tensor, non-zero = in -- ``otsu_mask(x).mask``,
    ``saturation_mask(x).mask``.  ``offset``: a non-negative int; another offset takes another sample where a group holds more than ``h * w``
    pixels.  The module docstring states the rule.  Three launches on the current stream (the rule: the mask launch in front), no
    synchronisation: the call can be captured in a graph.

    A slide: ``PixelSample.cat(*(sample_pixels(b, (64, 64), mask=otsu_mask(b).mask, pooled=True) for b in batches))``, then
    ``normaliser.estimate(s.pixels, pooled=True, mask=s.valid)`` once and ``apply`` per batch."""
    height, width = _check_size(size)
    fe.whole_number(offset, "offset must be an int in 0 .. 2^63 - 1", 0, (1 << 63) - 1)
    last, (n, h, w) = fe.image_4d(images, channel_axis, "sample_pixels")
    if images.dtype not in (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"sample_pixels: unsupported image dtype {images.dtype}")
    if h * w * (n if pooled else 1) > MAX_GROUP_PIXELS:
        raise ValueError(f"sample_pixels: a group must hold fewer than 2^31 pixels, got {n if pooled else 1} x {h} x {w}")
    threshold = masks.check_threshold(luminosity_threshold)
    device = images.device if images.device.type == "cuda" else torch.device("cuda")
    masked, explicit = masks.resolve(None, mask, n, h, w, device)
    from stainx_amd.backends.torch_hip_backend import sample_pixels_native, tissue_mask_native

    if masked and explicit is None:      # the rule: the mask launch in front, then the explicit path
        if images.device.type != "cuda":
            images = images.cuda()      # (once, for both calls)
        explicit = tissue_mask_native(images, threshold, last)[0]
    return PixelSample(*sample_pixels_native(images, explicit, height, width, bool(pooled), offset, last))
