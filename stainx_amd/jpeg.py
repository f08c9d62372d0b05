"""JPEG compression augmentation: a quality per tile, one fused launch (an extension: the reference has none).

Whole-slide images are stored JPEG-compressed at a quality and chroma subsampling that differ by scanner and site, and tiles are often
encoded once more when they are extracted; the 8 x 8 block artefacts and the smeared chroma are a known source of domain shift
(Schömig-Markiefka et al. 2021 stress-tested pathology models with it).  ``jpeg_compress`` returns what a tile looks like after one JPEG
round trip WITHOUT leaving the GPU: the lossy part of baseline JPEG as libjpeg implements it is 32-bit integer arithmetic and its entropy
coder is lossless, so encode and decode are fused in one launch (include/stainx_hip.h: sx_jpeg_roundtrip) and no bitstream is produced.
The result is, bit for bit, ``PIL.Image.save(..., "JPEG", quality=q, subsampling=s)`` followed by ``Image.open``.  ``JPEGAugment`` is the
``nn.Module`` beside ``GaussianBlurAugment``.

The rule: a uint8 byte is its level, a float element ``x`` is ``clamp(rint(255 x), 0, 255)`` (a NaN is level 0) -- a codec sees 8-bit
levels, this quantisation is part of the feature; JFIF colour conversion, 4:4:4 or 4:2:0 chroma, the "islow" integer DCT, Annex K's tables
scaled by the quality, the triangle chroma filter on the way back.  Every tile has ONE float32 ``quality``; NaN, infinite or ``< 1`` means
"leave this tile" (it is copied as ``adjust_hsv`` copies), a value above 100 is 100.  Quality 100 is NOT the identity: its tables are all
ones, but the colour conversion and the two transforms still round.
"""
from __future__ import annotations

from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks

SUBSAMPLING = {"444": 0, "420": 2, 0: 0, 2: 2}      # include/stainx_hip.h: Pillow's numbering
_ENGINES: dict[torch.device, Any] = {}      # (one engine per device for the module: the functional form has no object to keep it)


def _quality_rule(name: str, value: Any) -> int:
    return fe.whole_number(value, f"{name} must be an int in 1..100", 1, 100)


def _check_subsampling(subsampling: Any) -> int:
    if isinstance(subsampling, bool) or not isinstance(subsampling, (str, int)) or subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of '444', '420', 0, 2, got {subsampling!r}")
    return SUBSAMPLING[subsampling]


def _check_quality(quality: Any, n: int) -> int | None:
    """A tensor is checked by shape only (its values live on the device); an int by value.  -> the int, or None for a tensor."""
    if isinstance(quality, torch.Tensor):
        shape = tuple(quality.shape)
        if not (shape == () or (len(shape) == 1 and shape[0] in (1, n))):
            raise ValueError(f"quality must be an int or a tensor of shape (), (1,) or (N,) = ({n},), got {shape}")
        return None
    return _quality_rule("quality", quality)


def _jpeg(images: torch.Tensor, quality: Any, subsampling: int, who: str, *, mask: Any, mode: str | None, luminosity_threshold: float, channels_last: bool, normalize_to_0_1: bool,
          out_dtype: torch.dtype | None, device: torch.device | None) -> torch.Tensor:
    """The one path of both entry points; every argument error is raised before any GPU work."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    number = _check_quality(quality, dims[0])
    masked, explicit = fe.call_mask(mode, mask, single, dims, device or batch.device, channels_last, "JPEG round trip")
    run_on = fe.run_device(device, batch.device, who)
    engine = fe.held(_ENGINES, run_on, fe.engine, "JpegHIP")
    if number is not None:      # (a fill on the device, no host copy: the call stays capturable)
        quality = torch.full((1,), float(number), dtype=torch.float32, device=run_on)
    out = engine.apply(batch, quality, subsampling, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype, channels_last=channels_last,
                       masking=(explicit, luminosity_threshold) if masked else None)
    return out.squeeze(0) if single else out


def jpeg_compress(images: torch.Tensor, quality: Any, *, subsampling: Any = "420", mask: Any = None, channel_axis: int = 1, normalize_to_0_1: bool = False,
                  out_dtype: torch.dtype | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD) -> torch.Tensor:
    """The functional form: ``quality`` a Python int in 1..100 (checked here) or a tensor of shape (), (1,) or (N,) -- a quality per tile,
    read on the device, where NaN / infinite / ``< 1`` copies the tile and a value above 100 is 100 -- applied to CHW / NCHW tiles
    (``channel_axis=-1``: HWC / NHWC, unmasked only) on the GPU the tiles are on.  ``subsampling``: ``"420"`` (2) or ``"444"`` (0), one
    per call.  Quality 100 is not the identity (all-ones tables; the colour conversion and the DCT still round).  A float tile is
    quantised to 8-bit levels first.  ``mask``: an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W), or ``"luminosity"`` (the rule
    at ``luminosity_threshold``): only masked-in pixels are written from the round trip; the codec still reads every pixel.
    ``normalize_to_0_1``: uint8 tiles come out as float32 in [0, 1], float tiles are divided by 255; ``out_dtype``: bfloat16 / float16
    written directly from uint8 tiles.  One launch, no synchronisation."""
    return _jpeg(images, quality, _check_subsampling(subsampling), "jpeg_compress", mask=mask, mode=None, luminosity_threshold=masks.check_threshold(luminosity_threshold),
                 channels_last=fe.channels_last(channel_axis), normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


class JPEGAugment(nn.Module):
    """Random per-tile JPEG compression of CHW / NCHW tensors on an MI355X: per tile an integer quality drawn uniformly from ``lo..hi``
    inclusive with ``quality=(lo, hi)``, ``1 <= lo <= hi <= 100``; ``subsampling`` ``"420"`` or ``"444"`` for the module.  With probability
    ``1 - p`` a tile is left as it is (a NaN quality: it is copied, nothing is synchronised).  One launch per batch.
    ``normalize_to_0_1`` (default True, as ``HSVAugment``); ``generator`` drives ``sample_rows``; ``mask="luminosity"`` (or
    ``forward(..., mask=tensor)``): only tissue pixels are written from the round trip.  ``device=None`` follows the input tensor.  With a
    generator ON the device the qualities are drawn there and a call enqueues no host copy."""

    def __init__(self, quality: tuple[int, int] = (30, 95), *, subsampling: Any = "420", p: float = 1.0, device: str | torch.device | None = None, normalize_to_0_1: bool = True,
                 generator: torch.Generator | None = None, mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        super().__init__()
        if not isinstance(quality, (tuple, list)) or len(quality) != 2:
            raise ValueError(f"quality must be a (lo, hi) pair, got {quality!r}")
        self.quality = (_quality_rule("quality lo", quality[0]), _quality_rule("quality hi", quality[1]))
        if self.quality[0] > self.quality[1]:
            raise ValueError(f"quality must be a (lo, hi) pair with lo <= hi, got {tuple(quality)!r}")
        self.subsampling = _check_subsampling(subsampling)
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.device = fe.cuda_only(device, "JPEGAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator

    def sample_rows(self, n: int, device: str | torch.device | None = None) -> torch.Tensor:
        """(n,) float32 qualities on ``device``, drawn with the module's generator (on the generator's device, then moved), as
        ``GaussianBlurAugment.sample_rows`` draws: ``floor(lo + (hi + 1 - lo) * u)`` capped at ``hi``, ``u = rand(n)`` -- integers,
        uniform over ``lo..hi`` inclusive, exactly ``lo`` where ``lo == hi``.  ``p < 1``: one more draw, ``rand(n) < p``, in that order;
        a tile that is not chosen gets a NaN quality."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (n,), device).to(device)
        lo, hi = self.quality
        rows = torch.floor(lo + (hi + 1 - lo) * u).clamp(max=float(hi))
        if self.p < 1.0:
            rows = torch.where(fe.chosen(self.generator, n, self.p, device).squeeze(-1), rows, torch.full_like(rows, float("nan")))
        return rows

    def forward(self, img: torch.Tensor, rows: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``rows``: explicit (), (1,) or (N,) qualities (or an int) instead of a draw.  ``mask``: an explicit uint8 / bool tensor
        (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call; it wins over the module's rule."""
        if rows is None:      # (the draw comes first: the device is resolved before the mask is looked at)
            batch, _, (n, _, _) = fe.image_batch(img, False, "JPEGAugment")
            rows = self.sample_rows(n, fe.run_device(self.device, batch.device, "JPEGAugment"))
        return _jpeg(img, rows, self.subsampling, "JPEGAugment", mask=mask, mode=self.mask, luminosity_threshold=self.luminosity_threshold, channels_last=False,
                     normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device)

    def extra_repr(self) -> str:
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return f"quality={self.quality}, subsampling={self.subsampling}, p={self.p}, normalize_to_0_1={self.normalize_to_0_1}, mask={mask}"
