"""``LuminosityStandardizer``: staintools' ``LuminosityStandardizer.standardize`` on the device (an extension: the reference has none) --
the step staintools runs in front of every stain estimate.  Take a percentile of the lightness L*, scale L* so that the percentile
becomes white, clip at white, leave a* and b* alone (include/stainx_hip.h: sx_luminosity_percentile, sx_luminosity_apply).

The estimate is separate from the apply: a slide's percentile can be taken once (``estimate(thumbnail, pooled=True)``) and given to every
tile (``apply(tiles, estimate)``).  A per-tile percentile wrongly brightens a tile that is tissue edge to edge."""
from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch
from torch import nn

from stainx_amd import _frontend as fe


class LuminosityEstimate(NamedTuple):
    """``luminance``: (rows,) float32 on the device, the percentile of the linear-light luminance Y (NaN for an empty set); ``pixels``:
    (rows,) int64, the size of the set.  rows: one per tile, or 1 for a pooled estimate."""

    luminance: torch.Tensor
    pixels: torch.Tensor

    @property
    def lightness(self) -> torch.Tensor:
        """L* in 0..100, float64: ``116 f(Y) - 16`` with the conversion's ``f``."""
        y = self.luminance.to(torch.float64)
        f = torch.where(y > 0.008856, y.clamp_min(0.0).pow(1.0 / 3.0), 7.787 * y + 16.0 / 116.0)
        return 116.0 * f - 16.0


class LuminosityStandardizer(nn.Module):
    """Brightness standardisation: ``L*' = min(100 L* / L_p, 100)`` with ``L_p`` the ``percentile``-th percentile of L*; a* and b* are kept
    and nothing is quantised to 8 bits on the way.  ``statistics="tile"``: every tile's own percentile; ``"batch"``: one over the batch.

    The percentile is exact and deterministic: the nearest rank ``k = 1 + rint(0.01 * percentile * (|S| - 1))`` (half to even) of the
    float32 linear-light luminance over the set S, the rule of ``Vahadane.max_concentrations``.  This is NOT
    ``numpy.percentile(method="nearest")`` (the two ranks differ in a few cases per thousand), and NOT staintools' linear interpolation
    over 8-bit cv2 LAB values.  A pixel whose luminance is NaN is not in S.

    ``mask``: an explicit uint8 / bool (N, H, W) tensor that says which pixels ENTER S (pen marks kept out, say); every pixel is mapped,
    because the point of the step is that glass becomes white.  The ``"luminosity"`` rule is not offered as a mask here.  A tile whose
    set is empty, or whose percentile is black or exactly white (Y_p = 1: the gain is 1), is copied through.  Planar NCHW (or CHW) images of the five element types, on a ROCm
    device; there is no CPU path.  Nothing synchronises: a call can be captured in a graph."""

    def __init__(self, percentile: float = 95.0, statistics: str = "tile", device: str | torch.device | None = None):
        super().__init__()
        rule = "percentile must be a number in (0, 100]"
        self.percentile = fe.real_number(percentile, rule, rule, lambda v: not isinstance(percentile, bool) and math.isfinite(v) and 0.0 < v <= 100.0)
        if statistics not in ("tile", "batch"):
            raise ValueError(f"statistics must be 'tile' or 'batch', got {statistics!r}")
        self.statistics = statistics
        self.device = fe.cuda_only(device, "LuminosityStandardizer")
        self._engines: dict[torch.device, Any] = {}

    # ---- checks (all before any GPU work) ---------------------------------------------------------------------
    @staticmethod
    def _batch(images: Any) -> tuple[torch.Tensor, bool]:
        return fe.image_batch(images, False, "LuminosityStandardizer", tensor="a torch.Tensor")[:2]

    @staticmethod
    def _check_mask(mask: Any, batch: torch.Tensor, single: bool) -> torch.Tensor | None:
        """The standardiser's own mask rule: which pixels enter the set -- no ``"luminosity"`` mode and no (N, 1, H, W) shape."""
        if mask is None:
            return None
        if isinstance(mask, str):
            raise ValueError(f"mask must be an explicit uint8 / bool (N, H, W) tensor; the {mask!r} rule is not a mask mode of LuminosityStandardizer")
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"mask must be a uint8 / bool tensor, got {type(mask).__name__}" + (f" of {mask.dtype}" if isinstance(mask, torch.Tensor) else ""))
        mask = fe.tile_mask(mask, single)
        want = (batch.shape[0], batch.shape[2], batch.shape[3])
        if tuple(mask.shape) != want:
            raise ValueError(f"mask must have shape {want}, got {tuple(mask.shape)}")
        return mask

    def _engine(self, batch: torch.Tensor):
        device = fe.run_device(self.device, batch.device, "LuminosityStandardizer", fe.ON_TENSOR)
        return fe.held(self._engines, device, fe.engine, "LuminosityHIP")

    # ---- the public surface -----------------------------------------------------------------------------------
    def estimate(self, images: torch.Tensor, *, pooled: bool = False, mask: Any = None) -> LuminosityEstimate:
        """The percentile of every tile, or with ``pooled=True`` ONE over the batch (a slide's thumbnail, say)."""
        batch, single = self._batch(images)
        mask = self._check_mask(mask, batch, single)
        engine = self._engine(batch)
        return LuminosityEstimate(*engine.percentile(batch, self.percentile, pooled=bool(pooled), mask=mask))

    def apply(self, images: torch.Tensor, estimate: Any) -> torch.Tensor:
        """The map with a GIVEN estimate -- a ``LuminosityEstimate`` or a tensor of luminances -- of one row (every tile) or one row per tile."""
        batch, single = self._batch(images)
        luminance = estimate.luminance if isinstance(estimate, LuminosityEstimate) else estimate
        if not isinstance(luminance, torch.Tensor) or luminance.dim() > 1 or luminance.numel() not in (1, batch.shape[0]):
            raise ValueError(f"estimate must be a LuminosityEstimate or a tensor of 1 or {batch.shape[0]} luminances, got "
                             f"{tuple(luminance.shape) if isinstance(luminance, torch.Tensor) else type(luminance).__name__}")
        engine = self._engine(batch)
        out = engine.apply(batch, luminance)
        return out.squeeze(0) if single else out

    def forward(self, images: torch.Tensor, mask: Any = None) -> torch.Tensor:
        """``estimate`` then ``apply`` on the current stream (``statistics="batch"``: a pooled estimate)."""
        batch, single = self._batch(images)
        mask = self._check_mask(mask, batch, single)
        engine = self._engine(batch)
        batch = batch.to(engine.device).contiguous()
        luminance, _ = engine.percentile(batch, self.percentile, pooled=self.statistics == "batch", mask=mask)
        out = engine.apply(batch, luminance)
        return out.squeeze(0) if single else out

    standardize = forward

    def extra_repr(self) -> str:
        return f"percentile={self.percentile}, statistics={self.statistics!r}"
