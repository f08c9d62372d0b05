"""Histogram matching against a reference image (API of stainx.HistogramMatching, incl. ``channel_axis``)."""
from __future__ import annotations

from typing import Any

from stainx_amd import masks
from stainx_amd.normalizers._template import NormalizerTemplate


class HistogramMatching(NormalizerTemplate):
    """``statistics="batch"`` (the default, the reference's behaviour): one source histogram pooled over the whole batch.
    ``statistics="tile"`` (an extension; scikit-image's ``match_histograms`` on ONE image): one histogram and one lookup table per
    tile, three launches for the batch, tile t's result bit for bit that of transforming tile t alone.  ``fit`` is the same in both.

    ``mask="luminosity"`` (an extension, opt-in): the histograms -- of the reference in ``fit``, of the source in ``transform`` -- count
    TISSUE pixels only (a pixel is tissue iff L* / 100 < ``luminosity_threshold``; a pixel's three channels are in or out together), the
    lookup tables take the tissue count as their number of pixels, and background pixels are written with the bits of the input
    (floats are not quantised).  ``fit`` / ``transform`` / ``fit_transform`` also take ``mask=`` for one call: an explicit uint8 / bool
    tensor (N, H, W) or (N, 1, H, W) on the device, non-zero = tissue, which replaces the rule.  A tile or batch without tissue passes
    through unchanged.  The tissue edge is a hard edge: no seam smoothing.  ``mask=None`` is the unmasked library, bit for bit."""

    engine = "HistogramMatchingHIP"
    # three normalised 256-bin histograms (one per channel); `_reference_histogram` is the first of them, `_ref_vals` /
    # `_ref_cdf` exist for attribute compatibility with the reference and stay unset (its transform never reads them)
    fitted_slots = ("_ref_histograms_256", "_reference_histogram", "_ref_vals", "_ref_cdf")

    def __init__(self, device: Any | None = None, backend: str | None = None, channel_axis: int = 1, statistics: str = "batch", mask: str | None = None,
                 luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        if statistics not in ("batch", "tile"):
            raise ValueError(f"statistics must be 'batch' or 'tile', got {statistics!r}")
        self.statistics = statistics
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.channel_axis = channel_axis
        super().__init__(device=device, backend=backend)

    def engine_options(self) -> dict:
        return {"channel_axis": self.channel_axis}

    def learn(self, engine, images):
        per_channel = engine.compute_reference_histograms(images)
        return per_channel, per_channel[0], None, None

    def arguments(self) -> tuple:
        return (self._ref_histograms_256 if self._ref_histograms_256 else self._reference_histogram,)

    def _masking(self, images: Any, mask: Any, what: str) -> tuple[bool, Any]:
        """(masked call?, explicit mask or None), checked against the images before any GPU work."""
        if mask is None and self.mask is None:
            return False, None
        shape = tuple(getattr(images, "shape", ()))
        last = self.channel_axis == -1 or (self.channel_axis == 3 and len(shape) == 4)
        if len(shape) != 4 or shape[-1 if last else 1] != 3:
            raise ValueError(f"HistogramMatching {what} expects 4D images with 3 channels on axis {self.channel_axis}, got shape {shape}")
        n, h, w = (shape[0], shape[1], shape[2]) if last else (shape[0], shape[2], shape[3])
        return masks.resolve(self.mask, mask, n, h, w, self.device)

    def fit(self, images: Any, mask: Any = None) -> "HistogramMatching":
        masked, explicit = self._masking(images, mask, "fit")
        if not masked:
            return super().fit(images)
        per_channel = self._get_backend_impl().compute_reference_histograms_masked(images, explicit, self.luminosity_threshold)
        self._ref_histograms_256, self._reference_histogram, self._ref_vals, self._ref_cdf = per_channel, per_channel[0], None, None
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
