"""Vahadane stain normalisation (an extension: the reference has Macenko, Reinhard and histogram matching): the stain basis comes from
a sparse non-negative matrix factorisation of the optical density (Vahadane et al., IEEE TMI 2016; staintools' and tiatoolbox's
``VahadaneNormalizer``), everything downstream of the estimate is ``Macenko``'s."""
from __future__ import annotations

import math
from typing import Any

import torch

from stainx_amd import _frontend as fe, masks
from stainx_amd.normalizers.macenko import Macenko, StainEstimate, StainSeparation

MAX_ITERATIONS = 1000      # sx_vahadane_estimate: iterations in 1..1000


class Vahadane(Macenko):
    """H&E normalisation with Vahadane's stain estimate.  The estimate minimises ``0.5 |V - W H|^2 + regularizer |H|_1`` over a
    non-negative (3, 2) basis ``W`` with unit columns and non-negative concentrations ``H`` of the optical density ``V`` by exactly
    ``iterations`` rounds of (closed-form sparse coding per pixel, one block-coordinate sweep of the dictionary update) from ``init``:
    no early exit, so a call never synchronises, can be captured in a graph and gives the same bits every time.  haematoxylin is the
    column with the larger red optical density (staintools' rule).  ``max_concentrations`` are the 99th-percentile concentrations of
    the pseudo-inverse, as Macenko's: ``apply``, ``separate(source=...)`` and ``MacenkoAugment(source=..., normalizer=...)`` take a
    Vahadane estimate as they take Macenko's.

    ``mask="luminosity"`` is the default (staintools and tiatoolbox always estimate over the luminosity mask; glass pixels are copied
    through); ``mask=None`` estimates over every pixel; every method takes ``mask=`` for one call, as on ``Macenko``.  ``init``:
    ``"he"`` (the first two columns of ``stain_basis("he")``), a (3, 2) / (1, 3, 2) / (N, 3, 2) tensor or a ``StainEstimate`` (Macenko's,
    say).  A non-finite value under a masked-in pixel makes that group's estimate undefined; values under masked-out pixels never
    matter.  Planar NCHW images only."""

    engine = "VahadaneHIP"

    def __init__(self, device: Any | None = None, backend: str | None = None, normalize_to_0_1: bool = False, *, regularizer: float = 0.1, iterations: int = 30,
                 init: Any = "he", output_dtype: Any | None = None, mask: str | None = "luminosity", luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        self.regularizer = self._check_regularizer(regularizer)
        self.iterations = self._check_iterations(iterations)
        self.init = self._check_init(init)
        self._init_cache: dict = {}
        super().__init__(device=device, backend=backend, normalize_to_0_1=normalize_to_0_1, precision="stable", output_dtype=output_dtype, mask=mask,
                         luminosity_threshold=luminosity_threshold)

    # ---- checks (all before any GPU work) ---------------------------------------------------------------------
    @staticmethod
    def _check_regularizer(value: Any) -> float:
        rule = "regularizer must be a finite number >= 0"
        return fe.real_number(value, rule, rule, lambda v: math.isfinite(v) and v >= 0.0)

    @staticmethod
    def _check_iterations(value: Any) -> int:
        return fe.whole_number(value, f"iterations must be an integer in 1..{MAX_ITERATIONS}", 1, MAX_ITERATIONS)

    @staticmethod
    def _check_init(init: Any) -> Any:
        if isinstance(init, str):
            if init != "he":
                raise ValueError(f"init must be 'he', a (3, 2) / (1, 3, 2) / (N, 3, 2) tensor or a StainEstimate, got {init!r}")
            return init
        if isinstance(init, StainEstimate):
            init = init.stain_matrices
        shape = tuple(getattr(init, "shape", ()))
        if not isinstance(init, torch.Tensor) or not (shape == (3, 2) or (len(shape) == 3 and shape[1:] == (3, 2) and shape[0] >= 1)):
            raise ValueError(f"init must be 'he', a (3, 2) / (1, 3, 2) / (N, 3, 2) tensor or a StainEstimate, got {type(init).__name__} with shape {shape}")
        return init

    def _init_rows(self, rows: int, device: Any = None) -> torch.Tensor:
        """The initial bases as (1, 3, 2) or (rows, 3, 2) for a call on ``rows`` groups; with ``device``: float32 there, made once (a
        call inside a stream capture must not copy from host memory)."""
        if isinstance(self.init, str):
            from stainx_amd.deconv import stain_basis

            init = stain_basis("he")[:, :2].reshape(1, 3, 2) if device is None or device not in self._init_cache else None
        else:
            init = self.init.reshape(-1, 3, 2)
            if init.shape[0] not in (1, rows):
                raise ValueError(f"init holds {init.shape[0]} stain matrices; this call needs 1 or {rows}")
        if device is None:
            return init
        if device not in self._init_cache:
            self._init_cache[device] = init.to(device=device, dtype=torch.float32).contiguous()
        return self._init_cache[device]

    def _check_nchw(self, images: Any, what: str, channel_axis: int = 1) -> tuple[int, int, int]:
        if channel_axis not in (1, -3):
            raise ValueError(f"Vahadane {what} takes planar NCHW images only (channel_axis=1), got channel_axis={channel_axis}")
        return self._nchw(images, f"Vahadane {what}")

    def _dense_mask(self, engine, images: torch.Tensor, masked: bool, explicit: Any, luminosity_threshold: float) -> Any:
        """The mask of a masked call as ONE tensor for the calls that follow (the rule is evaluated once); None when unmasked."""
        if not masked:
            return None
        from stainx_amd import _native

        with _native.on_device(engine.device):
            return engine._mask_for(images, explicit, luminosity_threshold)

    def _prepare(self, images: Any, mask: Any, what: str):
        """(engine, dense device images, mask tensor or None) after the shape and mask checks."""
        masked, explicit = self._masking(images, mask, what)
        engine = self._get_backend_impl()
        images = images.to(engine.device).contiguous()
        return engine, images, self._dense_mask(engine, images, masked, explicit, self.luminosity_threshold)

    def _estimate(self, engine, images: torch.Tensor, mask: Any, pooled: bool) -> StainEstimate:
        rows = 1 if pooled else images.shape[0]
        out = engine.vahadane_estimate(images, self._init_rows(rows, engine.device), regularizer=self.regularizer, iterations=self.iterations, pooled=pooled, masked=mask is not None, mask=mask)
        return StainEstimate(out["he"], out["max_c"], None if pooled else out["pixels"].to(torch.float32))

    # ---- the public surface -----------------------------------------------------------------------------------
    def estimate(self, images: Any, *, pooled: bool = False, mask: Any = None, channel_axis: int = 1) -> StainEstimate:
        """Vahadane's stain basis of every tile of ``images`` (NCHW), or with ``pooled=True`` ONE basis over the batch (leading axis
        1), with the 99th-percentile concentrations of its pseudo-inverse.  ``tissue_pixels``: the pixels the estimate ran over, per
        tile (None when pooled).  A tile (or pooled batch) without a masked-in pixel gets NaN rows and 0 pixels, which ``apply`` with
        a mask treats as "copy the tile through".  Needs no ``fit()``."""
        shape = self._check_nchw(images, "estimate", channel_axis)
        self._init_rows(1 if pooled else shape[0])
        engine, images, dense = self._prepare(images, mask, "estimate")
        return self._estimate(engine, images, dense, bool(pooled))

    def max_concentrations(self, images: Any, stain_matrices: Any, *, pooled: bool = False, mask: Any = None, channel_axis: int = 1) -> torch.Tensor:
        """The (rows, 2) float32 99th-percentile concentrations (nearest rank) of GIVEN stain matrices -- (3, 2), (1, 3, 2) or one per
        row -- over each tile's (``pooled``: the batch's) masked-in pixels: what ``apply`` needs beside a basis that was estimated
        elsewhere (tiatoolbox, HistomicsTK).  Bit for bit the percentile of ``separate(source=(he, None), own_basis=True,
        concentrations=True)``'s concentrations."""
        shape = self._check_nchw(images, "max_concentrations", channel_axis)
        rows = 1 if pooled else shape[0]
        if isinstance(stain_matrices, StainEstimate):
            stain_matrices = stain_matrices.stain_matrices
        he_shape = tuple(getattr(stain_matrices, "shape", ()))
        if not isinstance(stain_matrices, torch.Tensor) or not (he_shape == (3, 2) or (len(he_shape) == 3 and he_shape[1:] == (3, 2) and he_shape[0] in (1, rows))):
            raise ValueError(f"stain_matrices must have shape (3, 2), (1, 3, 2) or ({rows}, 3, 2), got {he_shape}")
        engine, images, dense = self._prepare(images, mask, "max_concentrations")
        return engine.max_concentrations(images, stain_matrices, pooled=bool(pooled), masked=dense is not None, mask=dense)["max_c"]

    def fit(self, images: Any, mask: Any = None) -> "Vahadane":
        """The pooled estimate of the reference: ``_stain_matrix`` (3, 2) and ``_target_max_conc`` (2,)."""
        estimate = self.estimate(images, pooled=True, mask=mask)
        self._stain_matrix, self._target_max_conc = estimate.stain_matrices[0], estimate.max_concentrations[0]
        self._concentration_matrix = None
        self._is_fitted = True
        return self

    def transform(self, images: Any, mask: Any = None) -> Any:
        """Every tile's own estimate, then ``apply``: two library calls (and the rule's mask launch in front).  Under a mask, glass and
        tiles without an estimate are copied through."""
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        self._check_nchw(images, "transform")
        engine, images, dense = self._prepare(images, mask, "transform")
        estimate = self._estimate(engine, images, dense, False)
        if dense is None:
            return engine.apply(images, estimate.stain_matrices, estimate.max_concentrations, *self.arguments(), **self.call_options())
        return engine.apply_masked(images, estimate.stain_matrices, estimate.max_concentrations, *self.arguments(), dense, self.luminosity_threshold, **self.call_options())

    def separate(self, images: Any, *, stains: bool = True, concentrations: bool = False, own_basis: bool | None = None, source: Any = None, mask: Any = None) -> StainSeparation:
        """``Macenko.separate`` with Vahadane's per-tile estimate as the source where none is given."""
        if source is not None:
            return super().separate(images, stains=stains, concentrations=concentrations, own_basis=own_basis, source=source, mask=mask)
        if not (stains or concentrations):
            raise ValueError("separate: ask for stains, concentrations or both")
        if own_basis is not None and not own_basis and not self._is_fitted:
            raise ValueError("own_basis=False separates with the fitted reference: call fit() first")
        self._check_nchw(images, "separate")
        engine, images, dense = self._prepare(images, mask, "separate")
        estimate = self._estimate(engine, images, dense, False)
        # (dense is None only where neither the normaliser nor the call asks for a mask: the inherited call is unmasked then too)
        return super().separate(images, stains=stains, concentrations=concentrations, own_basis=own_basis, source=estimate, mask=dense)
