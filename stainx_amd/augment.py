"""``MacenkoAugment``: Macenko-space stain augmentation as an ``nn.Module`` (an extension: the reference has none).

The H&E jitter of Tellez et al., as torchstain's ``MacenkoAugmentor``, tiatoolbox's ``StainAugmentor`` and HistomicsTK's
``rgb_perturb_stain_concentration`` offer it: every tile is split into H and E concentrations in its own stain basis, they become
``alpha * C + beta`` with per-tile factors ``alpha ~ U[1 - sigma1, 1 + sigma1]``, ``beta ~ U[-sigma2, sigma2]``, and the tile is
rebuilt.  With a fitted reference (``reference=`` or ``normalizer=``) the tile is normalised to it and jittered in one call:
``C' = alpha * (C * target_max_conc / maxC) + beta`` rebuilt with the reference's stain matrix.  One library call per batch
(``MacenkoHIP.augment``, include/stainx_hip.h: sx_macenko_augment); the factors never leave the device.
"""
from __future__ import annotations

import math
from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks
from stainx_amd.normalizers import Macenko


class MacenkoAugment(nn.Module):
    """Random per-tile H&E concentration jitter of CHW / NCHW tensors on an MI355X.

    ``reference`` (fitted once, pooled over its tiles) or a fitted ``Macenko`` as ``normalizer`` selects normalise-and-jitter
    mode; with neither, every tile keeps its own stain basis.  ``device=None`` follows the input tensor.  ``normalize_to_0_1``
    (default True, as ``StainNormalizerTransform``): uint8 tiles come out as float32 in [0, 1], float tiles are divided by 255.
    ``generator`` drives ``sample_factors``; ``forward(img, alpha, beta)`` takes explicit (N, 2) factors instead.
    ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): the estimate is taken over the tissue pixels and only they are jittered;
    glass and pen marks are copied by the masked transform's background rule (``MacenkoHIP.augment_masked``).  ``source=`` (a
    ``StainEstimate``, or what ``Macenko.apply`` takes): the jitter with that GIVEN basis -- a slide's -- in one launch, no estimate
    (``MacenkoHIP.apply`` / ``apply_masked``), in own basis or normalised as the module's mode says.
    """

    def __init__(self, sigma1: float = 0.2, sigma2: float = 0.2, *, reference: torch.Tensor | None = None, normalizer: Macenko | None = None,
                 device: str | torch.device | None = None, normalize_to_0_1: bool = True, generator: torch.Generator | None = None,
                 mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD, source: Any = None):
        super().__init__()
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        sigma1, sigma2 = float(sigma1), float(sigma2)
        if not (math.isfinite(sigma1) and 0.0 <= sigma1 < 1.0):
            raise ValueError(f"sigma1 must lie in [0, 1) (alpha ~ U[1 - sigma1, 1 + sigma1] stays positive), got {sigma1}")
        if not (math.isfinite(sigma2) and sigma2 >= 0.0):
            raise ValueError(f"sigma2 must be a finite value >= 0, got {sigma2}")
        if reference is not None and normalizer is not None:
            raise ValueError("pass either reference= or normalizer=, not both")
        self.sigma1, self.sigma2 = sigma1, sigma2
        self.device = fe.cuda_only(device, "MacenkoAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator
        self._engines: dict[torch.device, Any] = {}
        if normalizer is not None:
            if not isinstance(normalizer, Macenko):
                raise ValueError(f"normalizer must be a stainx_amd.Macenko, got {type(normalizer).__name__}")
            if not getattr(normalizer, "_is_fitted", False):
                raise ValueError("normalizer must be fitted (call fit() first)")
        elif reference is not None:
            ref = fe.image_batch(reference, False, "MacenkoAugment")[0]
            target = fe.run_device(self.device, ref.device, "MacenkoAugment", fe.ON_TENSOR)
            normalizer = Macenko(device=target, backend="torch_hip").fit(ref.to(target))
        self.normalizer = normalizer
        # (the source's rows are checked against the batch in forward(); here: its kind, and that normalising has maxC to scale with)
        self.source = None if source is None else Macenko._check_source(source, self._source_rows(source), need_max_c=normalizer is not None)

    @staticmethod
    def _source_rows(source: Any) -> int:
        he = getattr(source, "stain_matrices", None)
        if he is None and isinstance(source, (tuple, list)) and len(source) > 0:
            he = source[0]
        shape = tuple(getattr(he, "shape", ()))
        return shape[0] if len(shape) == 3 else 1

    def sample_factors(self, n: int, device: str | torch.device | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(alpha, beta)``, each (n, 2) float32 on ``device``: ``alpha ~ U[1 - sigma1, 1 + sigma1]``, ``beta ~ U[-sigma2, sigma2]``
        (exactly 1 and 0 for sigma = 0), drawn with the module's generator (on the generator's device, then moved)."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (2, n, 2), device).to(device)
        alpha = 1.0 + self.sigma1 * (2.0 * u[0] - 1.0)
        beta = self.sigma2 * (2.0 * u[1] - 1.0)
        return alpha, beta

    def forward(self, img: torch.Tensor, alpha: torch.Tensor | None = None, beta: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``mask``: an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call; it wins
        over the module's rule.  All argument errors are raised before any GPU work."""
        batch, single, (n, h, w) = fe.image_batch(img, False, "MacenkoAugment")
        masked, explicit = fe.call_mask(self.mask, mask, single, (n, h, w), self.device or batch.device)
        given = None if self.source is None else Macenko._check_source(self.source, n, need_max_c=self.normalizer is not None)
        for name, factor in (("alpha", alpha), ("beta", beta)):
            if factor is not None and tuple(getattr(factor, "shape", ())) != (n, 2):
                raise ValueError(f"{name} must have shape (N, 2) = ({n}, 2), got {tuple(getattr(factor, 'shape', ()))}")
        device = fe.run_device(self.device, batch.device, "MacenkoAugment", fe.ON_TENSOR)
        if alpha is None or beta is None:
            drawn = self.sample_factors(n, device)
            alpha = drawn[0] if alpha is None else alpha
            beta = drawn[1] if beta is None else beta
        sm = tmc = None
        if self.normalizer is not None:
            sm, tmc = self.normalizer._stain_matrix.to(device), self.normalizer._target_max_conc.to(device)
        engine = fe.held(self._engines, device, fe.engine, "MacenkoHIP")
        batch = batch.to(device)
        if given is not None:      # (a given source basis: one launch, no estimate)
            he, max_c = given
            if masked:
                out = engine.apply_masked(batch, he, max_c, sm, tmc, explicit, self.luminosity_threshold, alpha=alpha, beta=beta, normalize_to_0_1=self.normalize_to_0_1)
            else:
                out = engine.apply(batch, he, max_c, sm, tmc, alpha=alpha, beta=beta, normalize_to_0_1=self.normalize_to_0_1)
        elif masked:
            out = engine.augment_masked(batch, alpha, beta, sm, tmc, explicit, self.luminosity_threshold, normalize_to_0_1=self.normalize_to_0_1)
        else:
            out = engine.augment(batch, alpha, beta, sm, tmc, normalize_to_0_1=self.normalize_to_0_1)
        return out.squeeze(0) if single else out

    def extra_repr(self) -> str:
        mode = "own basis" if self.normalizer is None else "normalise and jitter"
        source = "per-tile estimate" if self.source is None else f"given ({self._source_rows(self.source)} row{'s' if self._source_rows(self.source) != 1 else ''})"
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return f"sigma1={self.sigma1}, sigma2={self.sigma2}, mode={mode!r}, normalize_to_0_1={self.normalize_to_0_1}, mask={mask}, source={source!r}"
