"""Tone augmentation: per-tile brightness, contrast, gamma and additive Gaussian noise, and the grey statistics behind a contrast change
(an extension: the reference has none).

The "BC" member and the Gaussian noise of the augmentation set of Tellez et al. 2019: every channel of every pixel becomes
``t = clamp(a x + 255 b, 0, 255)``, then ``255 (t / 255)^gamma`` where ``gamma != 1``, then ``clamp(t + 255 sigma z, 0, 255)`` where noise
is asked for, with ONE row ``(a, b, gamma, sigma)`` and one 64-bit seed per tile -- a batch of tiles from different slides gets a draw per
tile.  ``z`` is a standard normal from a counter-based generator inside the kernel (Philox4x32-10, the pixel's index as the counter, the
tile's seed as the key, Box-Muller): the noise of a tile is a function of its seed alone -- the same for the tile alone and inside any
batch, in either layout, under any mask -- and no random tensor is written or read.  ``adjust_tone`` is one streaming launch per batch
(include/stainx_hip.h: sx_tone_apply) with rows and seeds in device memory; ``ToneAugment`` is the ``nn.Module`` beside ``HSVAugment``,
``GaussianNoiseAugment`` its noise-only form.  The arithmetic is float32 on 0-255 levels; uint8 results are ROUNDED to the nearest level, so
the identity row ``(1, 0, 1, 0)`` returns every byte.  A row with a NaN or an infinity, ``gamma <= 0`` or ``sigma < 0`` means "leave this
tile": it is copied.

A contrast change needs a pivot: the tile's mean grey level (torchvision's and PIL's rule).  ``grey_statistics`` returns the integer sums
behind it -- pixels, sum Y, sum Y^2 of ``grey_map``'s level per tile or per batch, in one launch that writes no map
(sx_grey_statistics) -- which are HistoQC's brightness and RMS-contrast measures as well (:class:`GreyStatistics`).
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks

IDENTITY_ROW = (1.0, 0.0, 1.0, 0.0)      # (a, b, gamma, sigma)
_ENGINES: dict[torch.device, Any] = {}      # (one engine per device: the functional forms have no object to keep it)


class GreyStatistics(NamedTuple):
    """The integer sums of the grey level (:func:`grey_statistics` returns it): three int64 tensors of shape ``(N,)``, or ``(1,)`` pooled
    over a batch, on the device.  ``pixels``: the pixels counted; ``sum``: sum Y; ``sum_squares``: sum Y^2."""

    pixels: torch.Tensor
    sum: torch.Tensor
    sum_squares: torch.Tensor

    @staticmethod
    def pool(*parts: "GreyStatistics") -> "GreyStatistics":
        """The sum of statistics of equal shapes, integer by integer (exact): the same tiles seen in several batches or on several ranks."""
        if not parts:
            raise ValueError("pool needs at least one GreyStatistics")
        shape = tuple(parts[0].pixels.shape)
        for item in parts:
            if not isinstance(item, GreyStatistics):
                raise ValueError(f"pool takes GreyStatistics, got {type(item).__name__}")
            if tuple(item.pixels.shape) != shape:
                raise ValueError(f"pool takes statistics of equal shapes, got {shape} and {tuple(item.pixels.shape)}")
        return GreyStatistics(*(torch.stack(list(words)).sum(dim=0) for words in zip(*parts)))

    def mean(self) -> torch.Tensor:
        """``sum / pixels`` in float64 on the device, on the 0-255 scale (HistoQC's brightness); NaN where ``pixels == 0``."""
        return self.sum.to(torch.float64) / self.pixels.to(torch.float64)

    def rms_contrast(self) -> torch.Tensor:
        """The population standard deviation of the grey level, ``sqrt(sum_squares / pixels - mean^2)``, in float64 on the device, on the
        0-255 scale; NaN where ``pixels == 0``."""
        pixels = self.pixels.to(torch.float64)
        mean = self.sum.to(torch.float64) / pixels
        return (self.sum_squares.to(torch.float64) / pixels - mean * mean).clamp_min(0.0).sqrt()


def _check_rows(rows: Any, n: int) -> None:
    shape = tuple(getattr(rows, "shape", ()))
    if not isinstance(rows, torch.Tensor) or not (shape == (4,) or (len(shape) == 2 and shape[1] == 4 and shape[0] in (1, n))):
        raise ValueError(f"rows must be a tensor of shape (4,), (1, 4) or (N, 4) = ({n}, 4) holding (a, b, gamma, sigma), got {shape}")


def _check_seeds(seeds: Any, n: int) -> None:
    if seeds is None:
        return
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int64 or tuple(seeds.shape) != (n,):
        raise ValueError(f"seeds must be None or an int64 tensor of shape (N,) = ({n},), got {getattr(seeds, 'dtype', type(seeds).__name__)} {tuple(getattr(seeds, 'shape', ()))}")


def _adjust(images: torch.Tensor, rows: torch.Tensor, seeds: torch.Tensor | None, who: str, *, shared_noise: bool, mask: Any, mode: str | None, luminosity_threshold: float,
            channels_last: bool, normalize_to_0_1: bool, out_dtype: torch.dtype | None, device: torch.device | None) -> torch.Tensor:
    """The one path of both entry points; every argument error is raised before any GPU work."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    _check_rows(rows, dims[0])
    _check_seeds(seeds, dims[0])
    masked, explicit = fe.call_mask(mode, mask, single, dims, device or batch.device, channels_last, "tone jitter")
    engine = fe.held(_ENGINES, fe.run_device(device, batch.device, who), fe.engine, "ToneHIP")
    out = engine.apply(batch, rows, seeds, shared_noise=shared_noise, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype, channels_last=channels_last,
                       masking=(explicit, luminosity_threshold) if masked else None)
    return out.squeeze(0) if single else out


def adjust_tone(images: torch.Tensor, rows: torch.Tensor, *, seeds: torch.Tensor | None = None, shared_noise: bool = False, mask: Any = None, channel_axis: int = 1,
                normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD) -> torch.Tensor:
    """The functional form: ``rows`` (4,), (1, 4) or (N, 4) floats ``(a, b, gamma, sigma)`` applied to CHW / NCHW tiles
    (``channel_axis=-1``: HWC / NHWC, unmasked only) on the GPU the tiles are on.  ``seeds``: (N,) int64 on the device, one per tile, or None:
    no noise whatever ``sigma`` says.  ``shared_noise``: one normal per pixel for the three channels (grey noise) instead of one per
    channel.  ``mask``, ``normalize_to_0_1``, ``out_dtype``, ``luminosity_threshold`` as for :func:`stainx_amd.adjust_hsv`.  One launch, no
    synchronisation; rows and seeds stay on the device."""
    return _adjust(images, rows, seeds, "adjust_tone", shared_noise=bool(shared_noise), mask=mask, mode=None, luminosity_threshold=masks.check_threshold(luminosity_threshold),
                   channels_last=fe.channels_last(channel_axis), normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


def _grey_statistics(batch: torch.Tensor, dims: tuple[int, int, int], mask: Any, mode: str | None, pooled: bool, last: bool, threshold: float, device: torch.device | None,
                     who: str) -> GreyStatistics:
    masked, explicit = fe.call_mask(mode, mask, False, dims, device or batch.device, last, "grey statistics call")
    engine = fe.held(_ENGINES, fe.run_device(device, batch.device, who), fe.engine, "ToneHIP")
    words = engine.statistics(batch, pooled=pooled, channels_last=last, masking=(explicit, threshold) if masked else None)
    return GreyStatistics(words[:, 0], words[:, 1], words[:, 2])


def grey_statistics(images: torch.Tensor, *, mask: Any = None, pooled: bool = False, channel_axis: int = 1,
                    luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD) -> GreyStatistics:
    """The integer sums of the grey level of a batch: :class:`GreyStatistics` of shape ``(N,)``, or ``(1,)`` with ``pooled=True``.  ``images``:
    NCHW (``channel_axis=-1``: NHWC, unmasked only) with C = 3 on the GPU.  Y is :func:`stainx_amd.grey_map`'s level; a pixel with a NaN channel
    has Y = 0 and is counted.  ``mask``: None (every pixel is counted), ``"luminosity"`` (the :func:`stainx_amd.tissue_mask` launch in front, at
    ``luminosity_threshold``) or an ``(N, H, W)`` / ``(N, 1, H, W)`` uint8 / bool tensor on the images' device: only masked-in pixels are
    counted.  One launch that reads the tiles once and writes no map (include/stainx_hip.h: sx_grey_statistics), no synchronisation."""
    threshold = masks.check_threshold(luminosity_threshold)
    last, dims = fe.image_4d(images, channel_axis, "grey_statistics")
    return _grey_statistics(images, dims, mask, None, bool(pooled), last, threshold, None, "grey_statistics")


def _magnitude(name: str, value: Any, upper: float | None, closed: bool = False) -> float:
    bound = "be a finite value >= 0" if upper is None else f"lie in [0, {upper}{']' if closed else ')'}"
    return fe.real_number(value, f"{name} must be a number", f"{name} must {bound}",
                          lambda v: math.isfinite(v) and v >= 0.0 and (upper is None or (v <= upper if closed else v < upper)))


class ToneAugment(nn.Module):
    """Random per-tile brightness, contrast, gamma and Gaussian noise of CHW / NCHW tensors on an MI355X.  Per tile it draws the intensity
    ratio ``r ~ U[1 - brightness, 1 + brightness]``, the contrast ``c ~ U[1 - contrast, 1 + contrast]``, the shift ``d ~ U[-shift, shift]``,
    ``gamma' = exp(U[-gamma, gamma])`` and ``sigma ~ U[0, noise]``; the row is ``a = c r``, ``b = (1 - c) r m / 255 + d``, ``gamma'``,
    ``sigma``: "brightness, then contrast about the brightened tile's mean" in ONE affine map, WITHOUT the clamp between the two that a
    chain of two torchvision / PIL calls has.  ``m`` is the tile's grey mean (``pivot="mean"``: one :func:`grey_statistics` launch in front;
    under the module's mask, the mean of the tissue; a tile with no counted pixel gets a NaN row and is copied), or ``255 pivot`` for a
    number (no statistics launch).  The rows are torch ops on the device; nothing is synchronised.  ``noise > 0``: one int64 seed per tile
    is drawn and the kernel's own generator makes the field (``shared_noise``: the same normal for the three channels).  With probability
    ``1 - p`` a tile is left as it is (a NaN row).  ``normalize_to_0_1`` (default True, as ``HSVAugment``); ``generator`` drives every
    draw; ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): only tissue pixels change.  ``device=None`` follows the input tensor.
    The defaults are this library's own, not a published table's."""

    def __init__(self, brightness: float = 0.2, contrast: float = 0.2, *, shift: float = 0.0, gamma: float = 0.0, noise: float = 0.0, shared_noise: bool = False,
                 pivot: Any = "mean", p: float = 1.0, device: str | torch.device | None = None, normalize_to_0_1: bool = True, generator: torch.Generator | None = None,
                 mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        super().__init__()
        self.brightness = _magnitude("brightness", brightness, 1.0)
        self.contrast = _magnitude("contrast", contrast, 1.0)
        self.shift = _magnitude("shift", shift, None)
        self.gamma = _magnitude("gamma", gamma, None)
        self.noise = _magnitude("noise", noise, None)
        self.shared_noise = bool(shared_noise)
        if isinstance(pivot, str):
            if pivot != "mean":
                raise ValueError(f"pivot must be 'mean' or a number in [0, 1], got {pivot!r}")
            self.pivot: Any = "mean"
        else:
            self.pivot = fe.real_number(pivot, "pivot must be 'mean' or a number in [0, 1]", "pivot must be 'mean' or a number in [0, 1]", lambda v: 0.0 <= v <= 1.0)
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.device = fe.cuda_only(device, type(self).__name__)
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator
        self._held: dict[torch.device, tuple[torch.Tensor, torch.Tensor]] = {}      # (the draw's centre and reach on a device: uploaded once)

    def sample_rows(self, n: int, means: torch.Tensor | None = None, device: str | torch.device | None = None) -> torch.Tensor:
        """(n, 4) float32 rows ``(a, b, gamma', sigma)`` on ``device``, drawn with the module's generator (on the generator's device, then
        moved): ``u = rand((n, 5))``, columns ``r, c, d, log gamma', sigma`` as ``centre + reach * (2 u - 1)`` -- exactly the identity row
        where every magnitude is 0.  ``means``: (n,) grey means on the 0-255 scale (``GreyStatistics.mean()``), the pivots; None: ``255
        pivot`` of a numeric pivot.  A NaN mean gives a NaN row.  ``p < 1``: one more draw, ``rand(n) < p``, in that order; a tile that is
        not chosen gets a NaN row."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (n, 5), device).to(device)
        centre, reach = fe.held(self._held, device, lambda device: tuple(torch.tensor(row, dtype=torch.float32, device=device) for row in (
            (1.0, 1.0, 0.0, 0.0, 0.5 * self.noise), (self.brightness, self.contrast, self.shift, self.gamma, 0.5 * self.noise))))
        draws = centre + reach * (2.0 * u - 1.0)
        r, c, d, log_gamma, sigma = draws.unbind(dim=1)
        if means is None:
            if self.pivot == "mean":
                raise ValueError("sample_rows needs the tiles' grey means (GreyStatistics.mean()) where pivot='mean'")
            pivot = self.pivot      # (m / 255 with m = 255 pivot)
        else:
            if not isinstance(means, torch.Tensor) or tuple(means.shape) != (n,):
                raise ValueError(f"means must be a tensor of shape (N,) = ({n},), got {tuple(getattr(means, 'shape', ()))}")
            pivot = means.to(device=device, dtype=torch.float32) / 255.0
        rows = torch.stack([c * r, (1.0 - c) * r * pivot + d, torch.exp(log_gamma), sigma.clamp_min(0.0)], dim=1)
        if self.p < 1.0:
            rows = torch.where(fe.chosen(self.generator, n, self.p, device), rows, torch.full_like(rows, float("nan")))
        return rows

    def sample_seeds(self, n: int, device: str | torch.device | None = None) -> torch.Tensor:
        """(n,) int64 seeds on ``device``: ``randint(0, 2^63 - 1)`` with the module's generator, on the generator's device, then moved."""
        device = fe.draw_device(device, self.device)
        return fe.draw_seeds(self.generator, n, device).to(device)

    def forward(self, img: torch.Tensor, rows: torch.Tensor | None = None, seeds: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``rows``: explicit (4,), (1, 4) or (N, 4) rows instead of a draw; ``seeds``: explicit (N,) int64 seeds instead of a draw.  ``mask``:
        an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call; it wins over the
        module's rule."""
        who = type(self).__name__
        if rows is None or (seeds is None and self.noise > 0.0):      # (the draws come first: rows, then the selection, then the seeds)
            batch, single, dims = fe.image_batch(img, False, who)
            device = fe.run_device(self.device, batch.device, who)
            if rows is None:
                means = None
                if self.pivot == "mean":
                    means = _grey_statistics(batch.to(device), dims, fe.tile_mask(mask, single), self.mask, False, False, self.luminosity_threshold, self.device, who).mean()
                rows = self.sample_rows(dims[0], means, device)
            if seeds is None and self.noise > 0.0:
                seeds = self.sample_seeds(dims[0], device)
        return _adjust(img, rows, seeds, who, shared_noise=self.shared_noise, mask=mask, mode=self.mask, luminosity_threshold=self.luminosity_threshold, channels_last=False,
                       normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device)

    def extra_repr(self) -> str:
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return (f"brightness={self.brightness}, contrast={self.contrast}, shift={self.shift}, gamma={self.gamma}, noise={self.noise}, shared_noise={self.shared_noise}, "
                f"pivot={self.pivot!r}, p={self.p}, normalize_to_0_1={self.normalize_to_0_1}, mask={mask}")


class GaussianNoiseAugment(ToneAugment):
    """Additive Gaussian noise alone: per tile ``sigma ~ U[sigma[0], sigma[1]]`` (on the [0, 1] scale) and one seed; every other magnitude
    is 0 and the pivot a number, so a call is ONE launch.  ``sigma``: a number (the upper end, from 0) or a ``(low, high)`` pair."""

    def __init__(self, sigma: Any = (0.0, 0.1), *, shared_noise: bool = False, p: float = 1.0, device: str | torch.device | None = None, normalize_to_0_1: bool = True,
                 generator: torch.Generator | None = None, mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        pair = tuple(sigma) if isinstance(sigma, (tuple, list)) else (0.0, sigma)
        if len(pair) != 2:
            raise ValueError(f"sigma must be a number or a (low, high) pair, got {sigma!r}")
        low, high = _magnitude("sigma", pair[0], None), _magnitude("sigma", pair[1], None)
        if low > high:
            raise ValueError(f"sigma must be a number or a (low, high) pair with low <= high, got {sigma!r}")
        super().__init__(0.0, 0.0, noise=high, shared_noise=shared_noise, pivot=0.5, p=p, device=device, normalize_to_0_1=normalize_to_0_1, generator=generator, mask=mask,
                         luminosity_threshold=luminosity_threshold)
        self.sigma = (low, high)

    def sample_rows(self, n: int, means: torch.Tensor | None = None, device: str | torch.device | None = None) -> torch.Tensor:
        """``ToneAugment.sample_rows`` with the drawn sigma moved into ``[low, high]``: ``low + (high - low) u``."""
        rows = super().sample_rows(n, None, device)
        low, high = self.sigma
        if low > 0.0:
            rows = torch.cat([rows[:, :3], low + rows[:, 3:] * ((high - low) / high)], dim=1)
        return rows
