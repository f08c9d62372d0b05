"""Histogram matching against a reference image (API of stainx.HistogramMatching, incl. ``channel_axis``)."""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe, masks
from stainx_amd.normalizers._template import NormalizerTemplate


class HistogramStatistics(NamedTuple):
    """Integer grey-level histograms of a source, estimated once and applied elsewhere (``HistogramMatching.estimate`` returns it,
    ``lookup_tables`` and ``apply`` take it).  ``counts``: (S, 3, 256) int64, bin b of channel c of set s; ``pixels``: (S,) int64, the
    pixels (with a mask: the tissue pixels) each channel of the set counted; both on the device.  S = N for a set per tile, 1 for one
    set pooled over a batch.

    Counts are integers, so histograms of different batches, slides or ranks ADD UP EXACTLY: :meth:`pool` adds any number of them into
    one set, and ``torch.distributed.all_reduce`` (SUM) on the two tensors pools them over ranks.  A lookup table built from added
    counts is, bit for bit, the table of the concatenated pixels."""

    counts: torch.Tensor
    pixels: torch.Tensor

    @staticmethod
    def pool(*stats: "HistogramStatistics") -> "HistogramStatistics":
        """One set, (1, 3, 256) and (1,): the sum of every set of every argument (a torch add where the tensors live; exact)."""
        if not stats:
            raise ValueError("pool needs at least one HistogramStatistics")
        counts = pixels = None
        for item in stats:
            c, p = _check_statistics(item)
            c, p = c.sum(dim=0, keepdim=True), p.sum(dim=0, keepdim=True)
            counts, pixels = (c, p) if counts is None else (counts + c, pixels + p)
        return HistogramStatistics(counts, pixels)


def _check_statistics(source: Any) -> tuple[torch.Tensor, torch.Tensor]:
    if not (isinstance(source, (tuple, list)) and len(source) == 2 and all(isinstance(t, torch.Tensor) for t in source)):
        raise ValueError("source must be a HistogramStatistics (counts, pixels) or a float32 table tensor")
    counts, pixels = source
    if counts.dim() != 3 or tuple(counts.shape[1:]) != (3, 256) or counts.shape[0] < 1:
        raise ValueError(f"source counts must have shape (S, 3, 256) with S >= 1, got {tuple(counts.shape)}")
    if tuple(pixels.shape) != (counts.shape[0],):
        raise ValueError(f"source pixels must have shape (S,) = ({counts.shape[0]},), got {tuple(pixels.shape)}")
    for name, value in (("counts", counts), ("pixels", pixels)):
        if value.dtype != torch.int64:
            raise ValueError(f"source {name} must have dtype int64, got {value.dtype}")
    return counts, pixels


class HistogramMatching(NormalizerTemplate):
    """``statistics="batch"`` (the default, the reference's behaviour): one source histogram pooled over the whole batch.
    ``statistics="tile"`` (an extension; scikit-image's ``match_histograms`` on ONE image): one histogram and one lookup table per
    tile, three launches for the batch, tile t's result bit for bit that of transforming tile t alone.  ``fit`` is the same in both.

    ``mask="luminosity"`` (an extension, opt-in): the histograms -- of the reference in ``fit``, of the source in ``transform`` -- count
    TISSUE pixels only (a pixel is tissue iff L* / 100 < ``luminosity_threshold``; a pixel's three channels are in or out together), the
    lookup tables take the tissue count as their number of pixels, and background pixels are written with the bits of the input
    (floats are not quantised).  ``fit`` / ``transform`` / ``fit_transform`` also take ``mask=`` for one call: an explicit uint8 / bool
    tensor (N, H, W) or (N, 1, H, W) on the device, non-zero = tissue, which replaces the rule.  A tile or batch without tissue passes
    through unchanged.  The tissue edge is a hard edge: no seam smoothing.  ``mask=None`` is the unmasked library, bit for bit.

    Slide level (an extension): ``estimate`` counts the histograms of a source without transforming it, ``HistogramStatistics.pool`` adds
    those of many batches, ``lookup_tables`` builds the tables once, and ``apply`` normalises every batch of the slide with them in ONE
    launch -- no histogram pass and no table launch per call."""

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

    def _check_images(self, images: Any, what: str) -> tuple[int, int, int]:
        """(n, h, w); ``channel_axis=3`` means channels-last for 4-D input only (on a 3-D image it is the reference's HWC axis)."""
        last = self.channel_axis == -1 or (self.channel_axis == 3 and len(getattr(images, "shape", ())) == 4)
        return fe.image_batch(images, last, "HistogramMatching", promote=False, tensor=None,
                              refusal=f"HistogramMatching {what} expects 4D images with 3 channels on axis {self.channel_axis}")[2]

    def _masking(self, images: Any, mask: Any, what: str, dims: tuple[int, int, int] | None = None) -> tuple[bool, Any]:
        """(masked call?, explicit mask or None), checked against the images (``dims``: where the caller has checked them) before any GPU work."""
        if mask is None and self.mask is None:
            return False, None
        return fe.call_mask(self.mask, mask, False, dims or self._check_images(images, what), self.device)

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

    # ---- slide level: estimate once, apply given tables -----------------------------------------------------------
    def estimate(self, images: Any, *, pooled: bool = False, mask: Any = None) -> HistogramStatistics:
        """The integer histograms of ``images``, without transforming them: every tile's own, ``counts`` (N, 3, 256) and ``pixels`` (N,) --
        or with ``pooled=True`` ONE set over the batch, (1, 3, 256) and (1,).  The slide-level workflow: estimate batch by batch (a
        thumbnail, a sample of tissue tiles, the whole slide), ``HistogramStatistics.pool`` them, ``lookup_tables`` once, ``apply`` to
        every batch.  Needs no ``fit()``.  With a mask (the normaliser's rule, or ``mask=`` for this call) only tissue pixels count."""
        masked, explicit = self._masking(images, mask, "estimate", self._check_images(images, "estimate"))
        counts, pixels = self._get_backend_impl().estimate_histograms(images, per_tile=not pooled, masked=masked, mask=explicit, luminosity_threshold=self.luminosity_threshold)
        return HistogramStatistics(counts, pixels)

    def lookup_tables(self, source: Any) -> torch.Tensor:
        """(S, 3, 256) float32 lookup tables that map the histograms of ``source`` (a ``HistogramStatistics``) to the fitted reference: row
        ``[s][c]`` is the table the transform builds from those counts, bit for bit.  One launch.  A set with ``pixels == 0`` (a source
        without tissue) gets the identity table, so that it leaves grey levels where they are -- the reference's arithmetic, which never
        meets zero pixels, would give a table of zeros (black)."""
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        counts, pixels = _check_statistics(source)
        return self._get_backend_impl().lookup_tables(counts, pixels, *self.arguments())

    def apply(self, images: Any, source: Any, mask: Any = None) -> Any:
        """Normalise ``images`` to the fitted reference with a GIVEN source: a float32 table tensor from ``lookup_tables`` -- (3, 256),
        (1, 3, 256) (one set for the batch) or (N, 3, 256) (set t serves tile t) -- in ONE kernel launch, a pixel read and a pixel
        written (include/stainx_hip.h: sx_hm_apply_tables); or a ``HistogramStatistics`` of 1 or N sets, whose tables are built first
        (two launches).  With a mask (the normaliser's rule, or ``mask=`` for this call) still one launch: tissue pixels get exactly the
        unmasked result, background pixels the bits of the input."""
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        dims = self._check_images(images, "apply")
        n = dims[0]
        masked, explicit = self._masking(images, mask, "apply", dims)
        if isinstance(source, torch.Tensor):
            shape = tuple(source.shape)
            if not (shape == (3, 256) or (len(shape) == 3 and shape[1:] == (3, 256) and shape[0] in (1, n))):
                raise ValueError(f"source tables must have shape (3, 256), (1, 3, 256) or (N, 3, 256) = ({n}, 3, 256), got {shape}")
            if source.dtype != torch.float32:
                raise ValueError(f"source tables must have dtype float32, got {source.dtype}")
            tables = source
        else:
            counts, pixels = _check_statistics(source)
            if counts.shape[0] not in (1, n):
                raise ValueError(f"source must have 1 or N = {n} rows of counts, got shape {tuple(counts.shape)}")
            tables = self._get_backend_impl().lookup_tables(counts, pixels, *self.arguments())
        if masked:
            return self._get_backend_impl().apply_tables_masked(images, tables, explicit, self.luminosity_threshold)
        return self._get_backend_impl().apply_tables(images, tables)
