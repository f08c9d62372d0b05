"""HSV colour augmentation: per-tile hue, saturation and value jitter (an extension: the reference has none).

The HSV-light / HSV-strong augmentation of Tellez et al. 2019 (the paper ``HEDAugment`` and ``MacenkoAugment`` cite), and the third
colour space of RandStainNA: every tile's hue is rotated by ``dh`` turns, its saturation becomes ``a_s * s + b_s`` and its value
``a_v * v + b_v`` (both clamped to [0, 1]), with ONE row ``(dh, a_s, b_s, a_v, b_v)`` per tile -- a batch of tiles from different slides
gets a draw per tile.  A jitter needs no statistics and no estimate: ``adjust_hsv`` is one streaming launch per batch (include/stainx_hip.h:
sx_hsv_apply) with the rows in device memory, and ``HSVAugment`` is the ``nn.Module`` beside ``HEDAugment``.  The arithmetic is float32 on
0-255 levels; uint8 results are ROUNDED to the nearest level (the stain transforms truncate), so the identity row ``(0, 1, 0, 1, 0)``
returns every uint8 colour exactly.  A row with a NaN or an infinity means "leave this tile": it is copied.  HSV *statistics*
(``StatisticsAugment(space="hsv")``) are not offered: hue is circular.
"""
from __future__ import annotations

import math
from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks

IDENTITY_ROW = (0.0, 1.0, 0.0, 1.0, 0.0)      # (dh, a_s, b_s, a_v, b_v)
_ENGINES: dict[torch.device, Any] = {}      # (one engine per device for the module: the functional form has no object to keep it)


def _check_rows(rows: Any, n: int) -> None:
    shape = tuple(getattr(rows, "shape", ()))
    if not isinstance(rows, torch.Tensor) or not (shape == (5,) or (len(shape) == 2 and shape[1] == 5 and shape[0] in (1, n))):
        raise ValueError(f"rows must be a tensor of shape (5,), (1, 5) or (N, 5) = ({n}, 5) holding (dh, a_s, b_s, a_v, b_v), got {shape}")


def _adjust(images: torch.Tensor, rows: torch.Tensor, who: str, *, mask: Any, mode: str | None, luminosity_threshold: float, channels_last: bool, normalize_to_0_1: bool,
            out_dtype: torch.dtype | None, device: torch.device | None) -> torch.Tensor:
    """The one path of both entry points; every argument error is raised before any GPU work."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    _check_rows(rows, dims[0])
    masked, explicit = fe.call_mask(mode, mask, single, dims, device or batch.device, channels_last, "HSV jitter")
    engine = fe.held(_ENGINES, fe.run_device(device, batch.device, who), fe.engine, "HsvHIP")
    out = engine.apply(batch, rows, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype, channels_last=channels_last,
                                masking=(explicit, luminosity_threshold) if masked else None)
    return out.squeeze(0) if single else out


def adjust_hsv(images: torch.Tensor, rows: torch.Tensor, *, mask: Any = None, channel_axis: int = 1, normalize_to_0_1: bool = False,
               out_dtype: torch.dtype | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD) -> torch.Tensor:
    """The functional form: ``rows`` (5,), (1, 5) or (N, 5) floats ``(dh, a_s, b_s, a_v, b_v)`` -- ``dh`` in turns -- applied to CHW /
    NCHW tiles (``channel_axis=-1``: HWC / NHWC, unmasked only) on the GPU the tiles are on.  ``mask``: an explicit uint8 / bool tensor
    (N, H, W) or (N, 1, H, W), or ``"luminosity"`` (the rule at ``luminosity_threshold``): only masked-in pixels change.
    ``normalize_to_0_1``: uint8 tiles come out as float32 in [0, 1], float tiles are divided by 255; ``out_dtype``: bfloat16 / float16
    written directly from uint8 tiles.  One launch, no synchronisation; the rows stay on the device."""
    return _adjust(images, rows, "adjust_hsv", mask=mask, mode=None, luminosity_threshold=masks.check_threshold(luminosity_threshold), channels_last=fe.channels_last(channel_axis),
                   normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


def _magnitude(name: str, value: Any, upper: float | None, closed: bool) -> float:
    bound = "be a finite value >= 0" if upper is None else f"lie in [0, {upper}{']' if closed else ')'}"
    return fe.real_number(value, f"{name} must be a number", f"{name} must {bound}",
                          lambda v: math.isfinite(v) and v >= 0.0 and (upper is None or (v <= upper if closed else v < upper)))


class HSVAugment(nn.Module):
    """Random per-tile HSV jitter ("HSV-light" with the defaults, Tellez et al.) of CHW / NCHW tensors on an MI355X: per tile
    ``dh ~ U[-hue, hue]`` turns, ``a_s ~ U[1 - saturation, 1 + saturation]``, ``b_s ~ U[-saturation_shift, saturation_shift]``, and
    ``a_v``, ``b_v`` likewise from ``value`` and ``value_shift``.  With probability ``1 - p`` a tile is left as it is (a NaN row: it is
    copied, nothing is synchronised).  One streaming launch per batch.  ``normalize_to_0_1`` (default True, as ``HEDAugment``);
    ``generator`` drives ``sample_rows``; ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): only tissue pixels are jittered.
    ``device=None`` follows the input tensor.  With a generator ON the device the rows are drawn there and a call enqueues no host
    copy."""

    def __init__(self, hue: float = 0.05, saturation: float = 0.1, value: float = 0.1, *, saturation_shift: float = 0.0, value_shift: float = 0.0, p: float = 1.0,
                 device: str | torch.device | None = None, normalize_to_0_1: bool = True, generator: torch.Generator | None = None, mask: str | None = None,
                 luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        super().__init__()
        self.hue = _magnitude("hue", hue, 0.5, True)
        self.saturation = _magnitude("saturation", saturation, 1.0, False)
        self.value = _magnitude("value", value, 1.0, False)
        self.saturation_shift = _magnitude("saturation_shift", saturation_shift, None, False)
        self.value_shift = _magnitude("value_shift", value_shift, None, False)
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.device = fe.cuda_only(device, "HSVAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator
        self._held: dict[torch.device, tuple[torch.Tensor, torch.Tensor]] = {}      # (the identity row and the magnitudes on a device: uploaded once)

    def sample_rows(self, n: int, device: str | torch.device | None = None) -> torch.Tensor:
        """(n, 5) float32 rows ``(dh, a_s, b_s, a_v, b_v)`` on ``device``, drawn with the module's generator (on the generator's
        device, then moved), as ``HEDAugment.sample_factors`` draws: ``identity + magnitude * (2 u - 1)``, ``u = rand((n, 5))`` -- exactly
        the identity row where every magnitude is 0.  ``p < 1``: one more draw, ``rand(n) < p``, in that order; a tile that is not chosen
        gets a NaN row."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (n, 5), device).to(device)
        magnitudes = (self.hue, self.saturation, self.saturation_shift, self.value, self.value_shift)
        identity, scale = fe.held(self._held, device, lambda device: tuple(torch.tensor(row, dtype=torch.float32, device=device) for row in (IDENTITY_ROW, magnitudes)))
        rows = identity + scale * (2.0 * u - 1.0)
        if self.p < 1.0:
            rows = torch.where(fe.chosen(self.generator, n, self.p, device), rows, torch.full_like(rows, float("nan")))
        return rows

    def forward(self, img: torch.Tensor, rows: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``rows``: explicit (5,), (1, 5) or (N, 5) rows instead of a draw.  ``mask``: an explicit uint8 / bool tensor (N, H, W) or
        (N, 1, H, W) on the device, or ``"luminosity"``, for this call; it wins over the module's rule."""
        if rows is None:      # (the draw comes first: the device is resolved before the mask is looked at)
            batch, _, (n, _, _) = fe.image_batch(img, False, "HSVAugment")
            rows = self.sample_rows(n, fe.run_device(self.device, batch.device, "HSVAugment"))
        return _adjust(img, rows, "HSVAugment", mask=mask, mode=self.mask, luminosity_threshold=self.luminosity_threshold, channels_last=False,
                       normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device)

    def extra_repr(self) -> str:
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return (f"hue={self.hue}, saturation={self.saturation}, value={self.value}, saturation_shift={self.saturation_shift}, value_shift={self.value_shift}, p={self.p}, "
                f"normalize_to_0_1={self.normalize_to_0_1}, mask={mask}")
