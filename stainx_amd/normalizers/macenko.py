"""Macenko stain normalisation (API of stainx.Macenko, incl. ``normalize_to_0_1`` and ``precision``)."""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe, masks
from stainx_amd.normalizers._template import NormalizerTemplate


class StainSeparation(NamedTuple):
    """What ``Macenko.separate`` returns (an extension; torchstain's ``normalize(..., stains=True)`` returns the first two).  A field
    that was not asked for is None.
    ``hematoxylin``, ``eosin``: (N, 3, H, W) images of one stain each, typed as ``transform`` types its output.
    ``concentrations``: (N, 2, H, W) float32, the (H, E) concentrations (normalised to the reference when one is used).
    ``stain_matrices``: (N, 3, 2) float32, each tile's own stain vectors ``HE_source``.
    ``max_concentrations``: (N, 2) float32, each tile's 99th-percentile concentrations ``maxC`` (with the reference only)."""

    hematoxylin: torch.Tensor | None
    eosin: torch.Tensor | None
    concentrations: torch.Tensor | None
    stain_matrices: torch.Tensor
    max_concentrations: torch.Tensor | None


class StainEstimate(NamedTuple):
    """A source stain basis, estimated once and applied elsewhere (``Macenko.estimate`` returns it, ``Macenko.apply`` takes it).
    ``stain_matrices``: (N, 3, 2) float32 ``HE_source`` per tile, or (1, 3, 2) for one basis pooled over a batch (a slide).
    ``max_concentrations``: (N, 2) or (1, 2) float32, the 99th-percentile concentrations ``maxC``.
    ``tissue_pixels``: (N,) float32, the pixels of each tile the optical-density filter kept (with a mask: of the masked-in pixels;
    0 for a tile without an estimate, whose rows are NaN); None for a pooled estimate."""

    stain_matrices: torch.Tensor
    max_concentrations: torch.Tensor
    tissue_pixels: torch.Tensor | None

    def complement(self) -> torch.Tensor:
        """The estimate as (N, 3, 3) -- pooled: (1, 3, 3) -- three-stain bases for ``ColorDeconvolution``: H, E and their normalised
        cross product (``stainx_amd.complement_basis``), so the part of the optical density outside the H&E plane becomes a third
        channel instead of being dropped.  On the estimate's device, no synchronisation."""
        from stainx_amd.deconv import complement_basis

        he = self.stain_matrices
        return complement_basis(he if he.dim() == 3 else he.unsqueeze(0))


class Macenko(NormalizerTemplate):
    """``normalize_to_0_1`` defaults to False here (output ~[0,255]); ``StainNormalizerTransform`` defaults it to True.
    ``precision`` takes the reference's two values, ``"stable"`` and ``"fast"``: both run the same exact kernels (fp64 covariance, exact
    nearest-rank percentiles) -- the reference's "fast" is a reduced-precision variant of its CUDA path (fp16 tensors, MAE ~0.05 grey
    levels), and the exact result lies inside its tolerance.  ``"sampled"`` is an extension (opt-in approximation: percentiles of a
    4096-pixel sample per tile, mean error ~0.5 / worst ~5 grey levels, about twice the throughput).

    ``mask="luminosity"`` (an extension, opt-in, as on ``Reinhard`` and ``HistogramMatching``): the estimate -- of the reference in
    ``fit``, of every tile in ``transform``, of ``estimate`` -- is the reference's algorithm run on the TISSUE pixels only (a pixel is
    tissue iff L* / 100 < ``luminosity_threshold``), and background pixels are copied (uint8 in, uint8 out: byte for byte).  The
    optical-density filter alone protects the stain vectors but not the concentration percentiles: on a tile that is mostly glass the
    99th percentile over all pixels is a much lower percentile of the tissue, and the tissue comes out too dark.  Every method also
    takes ``mask=`` for one call: an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W) on the device, non-zero = in, which replaces
    the rule (pen marks, folds, an annotated region).  For Macenko the rule is a ``tissue_mask()`` launch in front of the masked call
    -- one extra streaming pass over the images and its bytes; an explicit mask costs only its own bytes.  A tile with fewer than 3
    masked-in pixels has no estimate (NaN rows) and is copied through; the edge is hard.  A masked call always runs the exact four-pass
    form (``precision="sampled"`` with a mask is a ``ValueError``).  ``separate`` goes through the same rule (a masked-out pixel holds no
    stain) and ``MacenkoAugment`` has ``mask=`` of its own.  ``mask=None`` runs exactly the unmasked code."""

    engine = "MacenkoHIP"
    fitted_slots = ("_stain_matrix", "_target_max_conc", "_concentration_matrix")      # (3,2), (2,), unused

    def __init__(self, device: Any | None = None, backend: str | None = None, normalize_to_0_1: bool = False, precision: str = "stable", *,
                 output_dtype: Any | None = None, mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        if precision not in ("stable", "fast", "sampled"):
            raise ValueError(f"precision must be 'stable' or 'fast' (or the extension 'sampled'), got {precision!r}")
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        if self.mask is not None and precision == "sampled":
            raise ValueError("precision='sampled' has no masked form: a mask runs the exact four-pass estimate")
        self._precision = precision
        self.normalize_to_0_1 = normalize_to_0_1
        # extension (not in the reference): uint8 tiles come out as torch.bfloat16 / torch.float16, the `.to(dtype)` of the
        # result fused into the call; None keeps the reference's output type
        self.output_dtype = output_dtype
        super().__init__(device=device, backend=backend)

    def engine_options(self) -> dict:
        return {} if self._precision == "stable" else {"precision": self._precision}

    def learn(self, engine, images):
        stain_matrix, max_conc = engine.compute_reference_stain_matrix(images)
        return stain_matrix, max_conc, None

    def arguments(self) -> tuple:
        return (self._stain_matrix, self._target_max_conc)

    def call_options(self) -> dict:
        # the `/255` after the cast to the input dtype is fused into the last kernel
        options = {"normalize_to_0_1": bool(self.normalize_to_0_1)}
        if self.output_dtype is not None:
            options["out_dtype"] = self.output_dtype
        return options

    @staticmethod
    def _nchw(images: Any, who: str) -> tuple[int, int, int]:
        """(n, h, w) of planar images -- anything with a ``shape`` --, or ``who``'s refusal."""
        return fe.image_batch(images, False, who, promote=False, tensor=None, refusal=f"{who} expects NCHW images with C=3")[2]

    def _masking(self, images: Any, mask: Any, what: str) -> tuple[bool, Any]:
        """(masked call?, explicit mask or None) -- the call's ``mask=`` wins over the normaliser's rule --, checked before any GPU work."""
        if mask is None and self.mask is None:
            return False, None
        masked, explicit = fe.call_mask(self.mask, mask, False, self._nchw(images, f"Macenko {what}"), self.device)
        if masked and self._precision == "sampled":
            raise ValueError("precision='sampled' has no masked form: a mask runs the exact four-pass estimate")
        return masked, explicit

    def fit(self, images: Any, mask: Any = None) -> "Macenko":
        """``mask``: the reference's tissue (a tensor), for this call; a normaliser built with ``mask="luminosity"`` applies the rule."""
        masked, explicit = self._masking(images, mask, "fit")
        if not masked:
            return super().fit(images)
        self._stain_matrix, self._target_max_conc = self._get_backend_impl().compute_reference_stain_matrix_masked(images, explicit, self.luminosity_threshold)
        self._concentration_matrix = None
        self._is_fitted = True
        return self

    def fit_transform(self, images: Any, mask: Any = None) -> Any:
        return self.fit(images, mask=mask).transform(images, mask=mask)

    def transform(self, images: Any, mask: Any = None) -> Any:
        masked, explicit = self._masking(images, mask, "transform")
        if not masked:
            return super().transform(images)
        if not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        return self._get_backend_impl().transform_masked(images, *self.arguments(), explicit, self.luminosity_threshold, **self.call_options())

    def separate(self, images: Any, *, stains: bool = True, concentrations: bool = False, own_basis: bool | None = None, source: Any = None, mask: Any = None) -> StainSeparation:
        """Split every tile of ``images`` (NCHW) into its hematoxylin and eosin parts, with the transform's per-tile estimate.

        ``own_basis=None``: each tile's own stain basis while the normaliser is unfitted, the fitted reference once it is fitted --
        then ``C' = C * target_max_conc / maxC`` and the images are built with the reference's stain matrix (torchstain's ``H`` and
        ``E``).  ``own_basis=True`` forces the tile's own basis; ``False`` requires a fit.  The images follow ``normalize_to_0_1`` and
        ``output_dtype`` as ``transform`` does.  One library call (include/stainx_hip.h: sx_macenko_separate).

        ``source`` (what ``apply`` takes: a ``StainEstimate``, a ``StainSeparation`` or a ``(stain_matrices, max_concentrations)``
        pair, one row or N): separate with that GIVEN basis instead of each tile's own estimate -- one kernel launch, no estimate
        (sx_macenko_separate_apply); the returned ``stain_matrices`` / ``max_concentrations`` are the given ones, broadcast to N.
        With a mask (the normaliser's rule, or ``mask=`` for this call: a tensor or ``"luminosity"``) the estimate is taken over the
        masked-in pixels only, and a masked-out pixel -- and every pixel of a tile without an estimate -- holds no stain:
        concentrations 0, both images the level of zero concentration (240, typed and scaled as the tissue's levels)."""
        if not (stains or concentrations):
            raise ValueError("separate: ask for stains, concentrations or both")
        if self._precision == "sampled":
            raise ValueError("separate has no approximate form: use precision='stable' or 'fast' (both run the exact kernels)")
        if own_basis is None:
            own_basis = not self._is_fitted
        elif not own_basis and not self._is_fitted:
            raise ValueError("own_basis=False separates with the fitted reference: call fit() first")
        n = self._nchw(images, "Macenko separate")[0]
        given = None if source is None else self._check_source(source, n, need_max_c=not own_basis)
        masked, explicit = self._masking(images, mask, "separate")
        reference = (None, None) if own_basis else (self._stain_matrix, self._target_max_conc)
        engine = self._get_backend_impl()
        if given is not None and masked:
            out = engine.separate_apply_masked(images, *given, *reference, explicit, self.luminosity_threshold, stains=stains, concentrations=concentrations, **self.call_options())
        elif given is not None:
            out = engine.separate_apply(images, *given, *reference, stains=stains, concentrations=concentrations, **self.call_options())
        elif masked:
            out = engine.separate_masked(images, *reference, explicit, self.luminosity_threshold, stains=stains, concentrations=concentrations, **self.call_options())
        else:
            out = engine.separate(images, *reference, stains=stains, concentrations=concentrations, **self.call_options())
        images_out = out["stains"]
        return StainSeparation(images_out[0] if images_out is not None else None, images_out[1] if images_out is not None else None,
                               out["concentrations"], out["he"], out["max_c"])

    def estimate(self, images: Any, *, pooled: bool = False, mask: Any = None) -> StainEstimate:
        """The source stain basis of ``images`` (NCHW), without transforming them: every tile's own estimate (the transform's, exact
        percentiles), or with ``pooled=True`` ONE basis over all pixels of the batch -- the pooled fit that ``fit`` runs on a
        reference, returned with a leading axis of 1.  The slide-level workflow: estimate once (a thumbnail, a sample of tissue
        tiles), then ``apply`` the estimate to every tile.  Needs no ``fit()``.  With a mask (the normaliser's rule, or ``mask=`` for
        this call) the estimate is taken over the masked-in pixels only -- a thumbnail that is half glass --; a tile (or pooled batch)
        without an estimate gets NaN rows, which ``apply`` with a mask treats as "copy the tile through"."""
        if self._precision == "sampled":
            raise ValueError("estimate has no approximate form: use precision='stable' or 'fast' (both run the exact kernels)")
        self._nchw(images, "Macenko estimate")
        masked, explicit = self._masking(images, mask, "estimate")
        engine = self._get_backend_impl()
        if masked:
            out = engine.estimate_masked(images, explicit, self.luminosity_threshold, pooled=pooled)
            return StainEstimate(out["he"], out["max_c"], None if pooled else out["tissue"])
        if pooled:
            he, max_c = engine.compute_reference_stain_matrix(images)
            return StainEstimate(he.reshape(1, 3, 2), max_c.reshape(1, 2), None)
        out = engine.estimate(images)
        return StainEstimate(out["he"], out["max_c"], out["tissue"])

    @staticmethod
    def _check_source(source: Any, n: int, need_max_c: bool) -> tuple[Any, Any]:
        """``(stain_matrices, max_concentrations)`` of a given source basis for ``n`` tiles (``apply`` and ``separate`` take the same),
        with its shape checks -- before any GPU work."""
        if isinstance(source, (StainEstimate, StainSeparation)):
            he, max_c = source.stain_matrices, source.max_concentrations
        elif isinstance(source, (tuple, list)) and len(source) == 2:
            he, max_c = source
        else:
            raise ValueError("source must be a StainEstimate, a StainSeparation or a (stain_matrices, max_concentrations) pair")
        he_shape = tuple(getattr(he, "shape", ()))
        if not (he_shape == (3, 2) or (len(he_shape) == 3 and he_shape[1:] == (3, 2) and he_shape[0] in (1, n))):
            raise ValueError(f"source stain_matrices must have shape (3, 2), (1, 3, 2) or (N, 3, 2) = ({n}, 3, 2), got {he_shape}")
        n_sources = 1 if len(he_shape) == 2 else he_shape[0]
        if max_c is None:
            if need_max_c:
                raise ValueError("source carries no max_concentrations (a separation in its own basis?): they are needed to normalise to the reference")
        else:
            mc_shape = tuple(getattr(max_c, "shape", ()))
            if mc_shape != (n_sources, 2) and not (len(he_shape) == 2 and mc_shape == (2,)):
                raise ValueError(f"source max_concentrations must have shape ({n_sources}, 2) to match stain_matrices {he_shape}, got {mc_shape}")
        return he, max_c

    def apply(self, images: Any, source: Any, *, alpha: Any | None = None, beta: Any | None = None, own_basis: bool = False, mask: Any = None) -> Any:
        """Normalise ``images`` (NCHW) to the fitted reference with a GIVEN source basis instead of each tile's own estimate: one
        kernel launch, a pixel read and a pixel written (include/stainx_hip.h: sx_macenko_apply).

        ``source``: a ``StainEstimate``, a ``StainSeparation`` that carries ``max_concentrations``, or a ``(stain_matrices,
        max_concentrations)`` pair -- (3, 2) and (2,), or with a leading axis of 1 (one basis for the batch) or N (one per tile).
        ``alpha`` / ``beta`` (N, 2) jitter the (H, E) concentrations as ``MacenkoAugment`` does.  ``own_basis=True`` keeps the
        source's own stain vectors (no reference, no ``fit()``, ``max_concentrations`` may be None) and requires the factors.
        The output follows ``normalize_to_0_1`` and ``output_dtype`` as ``transform`` does.  With a mask (the normaliser's rule, or
        ``mask=`` for this call; include/stainx_hip.h: sx_macenko_apply_masked) masked-in pixels get exactly the unmasked result,
        masked-out pixels -- and tiles whose source row holds a NaN -- are copied."""
        if not own_basis and not self._is_fitted:
            raise ValueError("Must call fit() before transform()")
        if (alpha is None) != (beta is None):
            raise ValueError("alpha and beta go together: both or neither")
        if own_basis and alpha is None:
            raise ValueError("own_basis=True rebuilds every tile in the source's own basis: it needs the factors alpha and beta")
        n = self._nchw(images, "Macenko apply")[0]
        he, max_c = self._check_source(source, n, need_max_c=not own_basis)
        for name, factor in (("alpha", alpha), ("beta", beta)):
            if factor is not None and tuple(getattr(factor, "shape", ())) != (n, 2):
                raise ValueError(f"{name} must have shape (N, 2) = ({n}, 2), got {tuple(getattr(factor, 'shape', ()))}")
        reference = () if own_basis else (self._stain_matrix, self._target_max_conc)
        masked, explicit = self._masking(images, mask, "apply")
        if masked:
            return self._get_backend_impl().apply_masked(images, he, max_c, *(reference or (None, None)), explicit, self.luminosity_threshold, alpha=alpha, beta=beta,
                                                         **self.call_options())
        return self._get_backend_impl().apply(images, he, max_c, *reference, alpha=alpha, beta=beta, **self.call_options())
