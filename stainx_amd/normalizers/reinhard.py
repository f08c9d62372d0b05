"""Reinhard colour normalisation: LAB mean / standard deviation matching (API of stainx.Reinhard)."""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

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
    batch.  ``fit`` is the same in both modes."""

    engine = "ReinhardHIP"
    fitted_slots = ("_reference_mean", "_reference_std")      # LAB (3,) each, float32 on the device

    def __init__(self, device: Any | None = None, backend: str | None = None, statistics: str = "batch"):
        if statistics not in STATISTICS_MODES:
            raise ValueError(f"statistics must be 'batch' or 'tile', got {statistics!r}")
        self.statistics = statistics
        super().__init__(device=device, backend=backend)

    def learn(self, engine, images):
        return engine.compute_reference_mean_std(images)

    def transform(self, images: Any) -> Any:
        if self.statistics == "batch":
            return super().transform(images)
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        return self._get_backend_impl().transform_tiles(images, *self.arguments())

    @staticmethod
    def _check_images(images: Any, what: str) -> tuple:
        shape = tuple(getattr(images, "shape", ()))
        if len(shape) != 4 or shape[1] != 3:
            raise ValueError(f"Reinhard {what} expects NCHW images with C=3, got shape {shape}")
        return shape

    def estimate(self, images: Any, *, pooled: bool = False) -> ColorStatistics:
        """The LAB statistics of ``images`` (NCHW), without transforming them: every tile's own, (N, 3) each, in one statistics pass --
        or with ``pooled=True`` ONE set over all pixels of the batch, (1, 3) each (what ``fit`` computes on a reference).  The
        slide-level workflow: estimate once (a thumbnail, a sample of tissue tiles), then ``apply`` it to every tile.  Needs no ``fit()``."""
        self._check_images(images, "estimate")
        engine = self._get_backend_impl()
        if pooled:
            mean, std = engine.compute_reference_mean_std(images)
            return ColorStatistics(mean.reshape(1, 3), std.reshape(1, 3))
        return ColorStatistics(*engine.tile_statistics(images))

    def apply(self, images: Any, source: Any) -> Any:
        """Normalise ``images`` (NCHW) to the fitted reference with GIVEN source statistics: one kernel launch, a pixel read and a pixel
        written (include/stainx_hip.h: sx_reinhard_apply_stats).  ``source``: a ``ColorStatistics`` or a ``(mean, std)`` pair -- (3,),
        (1, 3) (one set for the batch) or (N, 3) (row t serves tile t)."""
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        n = self._check_images(images, "apply")[0]
        if isinstance(source, (tuple, list)) and len(source) == 2:      # (a ColorStatistics is a tuple of two)
            mean, std = source
        else:
            raise ValueError("source must be a ColorStatistics or a (mean, std) pair")
        shapes = []
        for name, value in (("mean", mean), ("std", std)):
            shape = tuple(getattr(value, "shape", ()))
            if not (shape == (3,) or (len(shape) == 2 and shape[1] == 3 and shape[0] in (1, n))):
                raise ValueError(f"source {name} must have shape (3,), (1, 3) or (N, 3) = ({n}, 3), got {shape}")
            shapes.append(1 if len(shape) == 1 else shape[0])
        if shapes[0] != shapes[1]:
            raise ValueError(f"source mean and std must have the same number of rows, got {shapes[0]} and {shapes[1]}")
        return self._get_backend_impl().apply_statistics(images, mean, std, *self.arguments())
