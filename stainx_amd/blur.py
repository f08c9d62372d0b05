"""Gaussian blur augmentation: a sigma per tile, one fused launch (an extension: the reference has none).

The blur of Tellez et al. 2019's augmentation set (the paper ``HEDAugment``, ``MacenkoAugment`` and ``HSVAugment`` cite), and the other half
of the focus measurement: a model that will see the blurred tiles ``focus_mask`` lets through has to be trained on blurred tiles, and a
focus cut is calibrated by blurring a slide's own sharp cells by a known sigma and reading ``laplacian_variance()`` again.  Every tile has
ONE float32 ``sigma``; ``gaussian_blur`` is one launch per batch (include/stainx_hip.h: sx_gaussian_blur) with the sigmas in device memory
and both passes of the separable filter on chip, and ``GaussianBlurAugment`` is the ``nn.Module`` beside ``HSVAugment``.

The rule: radius ``R = min(int(4 * sigma + 0.5), 16)`` of the float32 sigma (``scipy.ndimage.gaussian_filter`` with ``truncate=4.0``), taps
``exp(-i^2 / (2 sigma^2))`` divided by their sum, borders reflected without repeating the edge inside the tile (scipy's ``mode="mirror"``,
torch's ``reflect``), float32 arithmetic on the values as stored -- a uint8 byte is its level, a float element is taken as it is.  uint8
results are ROUNDED to the nearest level.  A sigma that is NaN, infinite, ``<= 0`` or below 0.125 (R = 0) means "leave this tile": it is
copied, bit for bit.  A finite sigma above ``MAX_SIGMA`` = 4 is 4.  A NaN pixel spreads over its ``(2R + 1)^2`` window.
"""
from __future__ import annotations

import math
from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks

MAX_SIGMA = 4.0      # include/stainx_hip.h: SX_BLUR_MAX_SIGMA
_ENGINES: dict[torch.device, Any] = {}      # (one engine per device for the module: the functional form has no object to keep it)


def _sigma_rule(name: str, value: Any) -> float:
    return fe.real_number(value, f"{name} must be a number", f"{name} must be finite and lie in [0, {MAX_SIGMA}]", lambda v: math.isfinite(v) and 0.0 <= v <= MAX_SIGMA)


def _check_sigma(sigma: Any, n: int) -> float | None:
    """A tensor is checked by shape only (its values live on the device); a number by value.  -> the number, or None for a tensor."""
    if isinstance(sigma, torch.Tensor):
        shape = tuple(sigma.shape)
        if not (shape == () or (len(shape) == 1 and shape[0] in (1, n))):
            raise ValueError(f"sigma must be a number or a tensor of shape (), (1,) or (N,) = ({n},), got {shape}")
        return None
    return _sigma_rule("sigma", sigma)


def _blur(images: torch.Tensor, sigma: Any, who: str, *, mask: Any, mode: str | None, luminosity_threshold: float, channels_last: bool, normalize_to_0_1: bool,
          out_dtype: torch.dtype | None, device: torch.device | None) -> torch.Tensor:
    """The one path of both entry points; every argument error is raised before any GPU work."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    number = _check_sigma(sigma, dims[0])
    masked, explicit = fe.call_mask(mode, mask, single, dims, device or batch.device, channels_last, "Gaussian blur")
    run_on = fe.run_device(device, batch.device, who)
    engine = fe.held(_ENGINES, run_on, fe.engine, "BlurHIP")
    if number is not None:      # (a fill on the device, no host copy: the call stays capturable)
        sigma = torch.full((1,), number, dtype=torch.float32, device=run_on)
    out = engine.apply(batch, sigma, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype, channels_last=channels_last,
                       masking=(explicit, luminosity_threshold) if masked else None)
    return out.squeeze(0) if single else out


def gaussian_blur(images: torch.Tensor, sigma: Any, *, mask: Any = None, channel_axis: int = 1, normalize_to_0_1: bool = False,
                  out_dtype: torch.dtype | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD) -> torch.Tensor:
    """The functional form: ``sigma`` a Python number (finite, ``0 <= sigma <= 4``, checked here; 0 copies) or a tensor of shape (),
    (1,) or (N,) -- a sigma per tile, read on the device, where NaN / infinite / ``<= 0`` copies the tile and a value above 4 is 4 --
    applied to CHW / NCHW tiles (``channel_axis=-1``: HWC / NHWC, unmasked only) on the GPU the tiles are on.  ``mask``: an explicit
    uint8 / bool tensor (N, H, W) or (N, 1, H, W), or ``"luminosity"`` (the rule at ``luminosity_threshold``): only masked-in pixels are
    written from the blur; the taps still read every pixel.  ``normalize_to_0_1``: uint8 tiles come out as float32 in [0, 1], float
    tiles are divided by 255; ``out_dtype``: bfloat16 / float16 written directly from uint8 tiles.  One launch, no synchronisation."""
    return _blur(images, sigma, "gaussian_blur", mask=mask, mode=None, luminosity_threshold=masks.check_threshold(luminosity_threshold), channels_last=fe.channels_last(channel_axis),
                 normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


class GaussianBlurAugment(nn.Module):
    """Random per-tile Gaussian blur of CHW / NCHW tensors on an MI355X: per tile ``sigma ~ U[lo, hi]`` with ``sigma=(lo, hi)``,
    ``0 <= lo <= hi <= 4``.  With probability ``1 - p`` a tile is left as it is (a NaN sigma: it is copied, nothing is synchronised), and
    so is a tile whose sigma falls below 0.125.  One launch per batch.  ``normalize_to_0_1`` (default True, as ``HSVAugment``);
    ``generator`` drives ``sample_rows``; ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): only tissue pixels are written from
    the blur.  ``device=None`` follows the input tensor.  With a generator ON the device the sigmas are drawn there and a call
    enqueues no host copy."""

    def __init__(self, sigma: tuple[float, float] = (0.1, 2.0), *, p: float = 1.0, device: str | torch.device | None = None, normalize_to_0_1: bool = True,
                 generator: torch.Generator | None = None, mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        super().__init__()
        if not isinstance(sigma, (tuple, list)) or len(sigma) != 2:
            raise ValueError(f"sigma must be a (lo, hi) pair, got {sigma!r}")
        self.sigma = (_sigma_rule("sigma lo", sigma[0]), _sigma_rule("sigma hi", sigma[1]))
        if self.sigma[0] > self.sigma[1]:
            raise ValueError(f"sigma must be a (lo, hi) pair with lo <= hi, got {tuple(sigma)!r}")
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.device = fe.cuda_only(device, "GaussianBlurAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator

    def sample_rows(self, n: int, device: str | torch.device | None = None) -> torch.Tensor:
        """(n,) float32 sigmas on ``device``, drawn with the module's generator (on the generator's device, then moved), as
        ``HSVAugment.sample_rows`` draws: ``lo + (hi - lo) * u``, ``u = rand(n)`` -- exactly ``lo`` where ``lo == hi``.  ``p < 1``: one
        more draw, ``rand(n) < p``, in that order; a tile that is not chosen gets a NaN sigma."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (n,), device).to(device)
        lo, hi = self.sigma
        rows = lo + (hi - lo) * u
        if self.p < 1.0:
            rows = torch.where(fe.chosen(self.generator, n, self.p, device).squeeze(-1), rows, torch.full_like(rows, float("nan")))
        return rows

    def forward(self, img: torch.Tensor, rows: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``rows``: explicit (), (1,) or (N,) sigmas (or a number) instead of a draw.  ``mask``: an explicit uint8 / bool tensor
        (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call; it wins over the module's rule."""
        if rows is None:      # (the draw comes first: the device is resolved before the mask is looked at)
            batch, _, (n, _, _) = fe.image_batch(img, False, "GaussianBlurAugment")
            rows = self.sample_rows(n, fe.run_device(self.device, batch.device, "GaussianBlurAugment"))
        return _blur(img, rows, "GaussianBlurAugment", mask=mask, mode=self.mask, luminosity_threshold=self.luminosity_threshold, channels_last=False,
                     normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device)

    def extra_repr(self) -> str:
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return f"sigma={self.sigma}, p={self.p}, normalize_to_0_1={self.normalize_to_0_1}, mask={mask}"
