"""Tissue masks for Reinhard and histogram matching: the luminosity rule as a call of its own, and the checks the normalisers share.

A mask has one value per pixel (a pixel's three channels are in or out together).  The rule (``mask="luminosity"``; staintools'
``LuminosityThresholdTissueLocator``, tiatoolbox): a pixel is tissue iff L* / 100 < ``luminosity_threshold``, L* of the pixel's unit value
(``u8 / 255``, floats as they are).  An explicit mask is a dense uint8 / bool tensor ``(N, H, W)`` or ``(N, 1, H, W)`` on the
normaliser's device, non-zero = tissue.  Every kernel decides a pixel with the same device function (csrc/tissue.hpp), so the rule and
a mask made by :func:`tissue_mask` give the same bits everywhere.
"""
from __future__ import annotations

import math
from typing import Any

import torch

MASK_MODES = ("luminosity",)
DEFAULT_LUMINOSITY_THRESHOLD = 0.8


def check_threshold(luminosity_threshold: Any) -> float:
    try:
        value = float(luminosity_threshold)
    except (TypeError, ValueError):
        raise ValueError(f"luminosity_threshold must be a number in (0, 1), got {luminosity_threshold!r}") from None
    if math.isnan(value) or not 0.0 < value < 1.0:
        raise ValueError(f"luminosity_threshold must lie in (0, 1), got {luminosity_threshold!r}")
    return value


def check_mask_mode(mask: Any) -> str | None:
    """The constructor's ``mask=``: None (no mask) or the name of a rule."""
    if mask is None:
        return None
    if not isinstance(mask, str) or mask not in MASK_MODES:
        hint = " (an explicit mask tensor belongs to the call: fit / transform / estimate / apply(..., mask=tensor))" if isinstance(mask, torch.Tensor) else ""
        raise ValueError(f"mask must be None or one of {list(MASK_MODES)}, got {mask if isinstance(mask, str) else type(mask).__name__!r}{hint}")
    return mask


def check_mask_tensor(mask: Any, n: int, h: int, w: int, device: Any) -> None:
    """An explicit mask for a call on ``n`` tiles of ``h x w`` pixels by a normaliser on ``device``: ValueError before any GPU work."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be None, 'luminosity' or a uint8 / bool tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask dtype must be uint8 or bool (non-zero = tissue), got {mask.dtype}")
    if tuple(mask.shape) not in ((n, h, w), (n, 1, h, w)):
        raise ValueError(f"mask shape must be (N, H, W) = ({n}, {h}, {w}) or (N, 1, H, W), got {tuple(mask.shape)}")
    want = torch.device(device)
    if mask.device.type != want.type or (want.index is not None and mask.device.index is not None and mask.device.index != want.index):
        raise ValueError(f"mask device must be the normaliser's device ({want}), got {mask.device}")


def resolve(mode: str | None, mask: Any, n: int, h: int, w: int, device: Any) -> tuple[bool, torch.Tensor | None]:
    """(masked call?, explicit mask or None) for a call: the call's ``mask=`` (a tensor, or the name of a rule) wins over the normaliser's mode."""
    if isinstance(mask, str):
        check_mask_mode(mask)
        return True, None
    if mask is not None:
        check_mask_tensor(mask, n, h, w, device)
        return True, mask
    return mode is not None, None


def tissue_mask(images: torch.Tensor, luminosity_threshold: float = DEFAULT_LUMINOSITY_THRESHOLD, *, channel_axis: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """The luminosity rule on a batch: ``(mask, counts)`` -- ``mask`` (N, H, W) uint8, 1 = tissue, and ``counts`` (N,) int64 tissue pixels per
    tile, both on the device.  ``images``: NCHW (``channel_axis=-1``: NHWC) with C = 3, any supported element type; a CPU tensor is moved
    to the current GPU.  One streaming kernel (include/stainx_hip.h: sx_tissue_mask)."""
    threshold = check_threshold(luminosity_threshold)
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"tissue_mask expects a 4-D image tensor, got {type(images).__name__} with shape {tuple(getattr(images, 'shape', ()))}")
    last = channel_axis in (-1, 3)
    if not last and channel_axis not in (1, -3):
        raise ValueError(f"Unsupported channel_axis={channel_axis}")
    if images.shape[-1 if last else 1] != 3:
        raise ValueError(f"tissue_mask expects 3 channels on axis {channel_axis}, got shape {tuple(images.shape)}")
    from stainx_amd.backends.torch_hip_backend import tissue_mask_native

    return tissue_mask_native(images, threshold, last)
