"""Reinhard colour normalisation: LAB mean / standard deviation matching (API of stainx.Reinhard)."""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe, masks
from stainx_amd.normalizers._template import NormalizerTemplate

STATISTICS_MODES = ("batch", "tile")


class ColorStatistics(NamedTuple):
    """LAB statistics of a source, estimated once and applied elsewhere (``Reinhard.estimate`` returns it, ``Reinhard.apply`` takes it).
    ``mean``, ``std``: (N, 3) float32 per tile, or (1, 3) for one set pooled over a batch (a slide); LAB on the reference's 0..255 scale,
    ``std`` unbiased -- what ``fit`` stores for the reference."""

    mean: torch.Tensor
    std: torch.Tensor


class Reinhard(NormalizerTemplate):
    """``statistics="batch"`` (the default, the reference's behaviour): the source mean / standard deviation are pooled over the whole
    batch.  ``statistics="tile"`` (an extension; what torchstain, tiatoolbox and HistomicsTK do with ONE image): every tile of a batch
    is normalised with its own statistics, still in two streaming launches, and its output does not depend on its neighbours in the
    batch.  ``fit`` is the same in both modes.

    ``mask="luminosity"`` (an extension, opt-in; HistomicsTK's ``reinhard(mask_out=)``, staintools' and tiatoolbox's tissue locator): the
    statistics -- of the reference in ``fit``, of the source in ``transform`` / ``estimate`` -- are taken over TISSUE pixels only (a pixel
    is tissue iff L* / 100 < ``luminosity_threshold``), and background pixels are written with the bits of the input.  Every method also
    takes ``mask=`` for one call: an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W) on the device, non-zero = tissue, which
    replaces the rule (also on a normaliser built with ``mask=None``).  A tile (``statistics="tile"``) or batch with fewer than two tissue
    pixels has no statistics (NaN) and passes through unchanged.  The tissue edge is a hard edge: there is no seam smoothing and no
    ``background=`` switch.  ``mask=None`` is the unmasked library, bit for bit."""

    engine = "ReinhardHIP"
    fitted_slots = ("_reference_mean", "_reference_std")      # LAB (3,) each, float32 on the device

    def __init__(self, device: Any | None = None, backend: str | None = None, statistics: str = "batch", mask: str | None = None,
                 luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        if statistics not in STATISTICS_MODES:
            raise ValueError(f"statistics must be 'batch' or 'tile', got {statistics!r}")
        self.statistics = statistics
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        super().__init__(device=device, backend=backend)

    def learn(self, engine, images):
        return engine.compute_reference_mean_std(images)

    def _masking(self, images: Any, mask: Any, what: str) -> tuple[bool, Any]:
        """(masked call?, explicit mask or None), checked against the images before any GPU work."""
        if mask is None and self.mask is None:
            return False, None
        return fe.call_mask(self.mask, mask, False, self._check_images(images, what), self.device)

    def fit(self, images: Any, mask: Any = None) -> "Reinhard":
        """``mask``: the reference's tissue (a tensor), for this call; a normaliser built with ``mask="luminosity"`` applies the rule."""
        masked, explicit = self._masking(images, mask, "fit")
        if not masked:
            return super().fit(images)
        mean, std, _ = self._get_backend_impl().masked_statistics(images, explicit, self.luminosity_threshold, per_tile=False)
        self._reference_mean, self._reference_std = mean[0], std[0]
        self._is_fitted = True
        return self

    def fit_transform(self, images: Any, mask: Any = None) -> Any:
        return self.fit(images, mask=mask).transform(images, mask=mask)

    def transform(self, images: Any, mask: Any = None) -> Any:
        masked, explicit = self._masking(images, mask, "transform")
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        if masked:
            return self._get_backend_impl().transform_masked(images, *self.arguments(), explicit, self.luminosity_threshold, per_tile=self.statistics == "tile")
        if self.statistics == "batch":
            return super().transform(images)
        return self._get_backend_impl().transform_tiles(images, *self.arguments())

    @staticmethod
    def _check_images(images: Any, what: str) -> tuple[int, int, int]:
        return fe.image_batch(images, False, "Reinhard", promote=False, tensor=None, refusal=f"Reinhard {what} expects NCHW images with C=3")[2]

    def estimate(self, images: Any, *, pooled: bool = False, mask: Any = None) -> ColorStatistics:
        """The LAB statistics of ``images`` (NCHW), without transforming them: every tile's own, (N, 3) each, in one statistics pass --
        or with ``pooled=True`` ONE set over all pixels of the batch, (1, 3) each (what ``fit`` computes on a reference).  The
        slide-level workflow: estimate once (a thumbnail, a sample of tissue tiles), then ``apply`` it to every tile.  Needs no ``fit()``.
        With a mask (the normaliser's rule, or ``mask=`` for this call) the statistics are those of the tissue pixels; a tile (or pooled
        batch) with fewer than two of them gets a row of NaN, which ``apply`` treats as "copy the tile through"."""
        self._check_images(images, "estimate")
        masked, explicit = self._masking(images, mask, "estimate")
        engine = self._get_backend_impl()
        if masked:
            mean, std, _ = engine.masked_statistics(images, explicit, self.luminosity_threshold, per_tile=not pooled)
            return ColorStatistics(mean, std)
        if pooled:
            mean, std = engine.compute_reference_mean_std(images)
            return ColorStatistics(mean.reshape(1, 3), std.reshape(1, 3))
        return ColorStatistics(*engine.tile_statistics(images))

    def apply(self, images: Any, source: Any, mask: Any = None, *, target: Any = None) -> Any:
        """Normalise ``images`` (NCHW) to the fitted reference with GIVEN source statistics: one kernel launch, a pixel read and a pixel
        written (include/stainx_hip.h: sx_reinhard_apply_stats).  ``source``: a ``ColorStatistics`` or a ``(mean, std)`` pair -- (3,),
        (1, 3) (one set for the batch) or (N, 3) (row t serves tile t).  With a mask (the normaliser's rule, or ``mask=`` for this call)
        still one launch: tissue pixels get exactly the unmasked result, background pixels -- and tiles whose row holds a NaN -- are copied.

        ``target`` (a ``ColorStatistics`` or ``(mean, std)`` pair of the same shapes): normalise to THESE statistics instead of the
        fitted reference -- a target per tile or per slide, no ``fit()`` needed; still one launch (sx_reinhard_apply_targets).  With one
        finite target row the bits are those of the fitted path with that reference; a tile whose source or target row holds a NaN is
        copied bit for bit, masked or not."""
        if target is None and not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        n = self._check_images(images, "apply")[0]
        masked, explicit = self._masking(images, mask, "apply")
        mean, std = fe.mean_std_rows(source, n, "source", "ColorStatistics", tensors=False)
        if target is not None:
            t_mean, t_std = fe.mean_std_rows(target, n, "target", "ColorStatistics", tensors=False)
            if masked:
                return self._get_backend_impl().apply_targets_masked(images, mean, std, t_mean, t_std, explicit, self.luminosity_threshold)
            return self._get_backend_impl().apply_targets(images, mean, std, t_mean, t_std)
        if masked:
            return self._get_backend_impl().apply_statistics_masked(images, mean, std, *self.arguments(), explicit, self.luminosity_threshold)
        return self._get_backend_impl().apply_statistics(images, mean, std, *self.arguments())
