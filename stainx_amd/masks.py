"""Tissue masks for Reinhard and histogram matching: the luminosity rule as a call of its own, and the checks the normalisers share.

A mask has one value per pixel (a pixel's three channels are in or out together).  The rule (``mask="luminosity"``; staintools'
``LuminosityThresholdTissueLocator``, tiatoolbox): a pixel is tissue iff L* / 100 < ``luminosity_threshold``, L* of the pixel's unit value
(``u8 / 255``, floats as they are).  An explicit mask is a dense uint8 / bool tensor ``(N, H, W)`` or ``(N, 1, H, W)`` on the
normaliser's device, non-zero = tissue.  Every kernel decides a pixel with the same device function (csrc/tissue.hpp), so the rule and
a mask made by :func:`tissue_mask` give the same bits everywhere.

Tissue detection (the second half of the file): :func:`luminosity_histogram`, :func:`otsu_threshold`, :func:`otsu_mask` -- a threshold taken
from the data -- and :func:`mask_morphology`, :func:`refine_mask` -- opening and closing of a mask; :func:`mask_components`,
:func:`remove_small_objects`, :func:`remove_small_holes` -- connected components and the filters by area that morphology cannot do.

Saturation-channel detection (the end of the file; CLAM's ``segmentTissue``): :func:`saturation_map`, :func:`median_filter`,
:func:`level_histogram`, :func:`otsu_level`, :func:`level_mask` and the pipeline :func:`saturation_mask` -- "is the pixel coloured" where the
luminosity rule asks "is the pixel dark".
"""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe

MASK_MODES = ("luminosity",)
DEFAULT_LUMINOSITY_THRESHOLD = 0.8


def check_threshold(luminosity_threshold: Any) -> float:
    return fe.real_number(luminosity_threshold, "luminosity_threshold must be a number in (0, 1)", "luminosity_threshold must lie in (0, 1)", lambda v: 0.0 < v < 1.0)


def check_mask_mode(mask: Any) -> str | None:
    """The constructor's ``mask=``: None (no mask) or the name of a rule."""
    if mask is None:
        return None
    if not isinstance(mask, str) or mask not in MASK_MODES:
        hint = " (an explicit mask tensor belongs to the call: fit / transform / estimate / apply(..., mask=tensor))" if isinstance(mask, torch.Tensor) else ""
        raise ValueError(f"mask must be None or one of {list(MASK_MODES)}, got {mask if isinstance(mask, str) else type(mask).__name__!r}{hint}")
    return mask


def check_mask_tensor(mask: Any, n: int, h: int, w: int, device: Any) -> None:
    """An explicit mask for a call on ``n`` tiles of ``h x w`` pixels by a normaliser on ``device``: ValueError before any GPU work."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be None, 'luminosity' or a uint8 / bool tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask dtype must be uint8 or bool (non-zero = tissue), got {mask.dtype}")
    if tuple(mask.shape) not in ((n, h, w), (n, 1, h, w)):
        raise ValueError(f"mask shape must be (N, H, W) = ({n}, {h}, {w}) or (N, 1, H, W), got {tuple(mask.shape)}")
    want = torch.device(device)
    if mask.device.type != want.type or (want.index is not None and mask.device.index is not None and mask.device.index != want.index):
        raise ValueError(f"mask device must be the normaliser's device ({want}), got {mask.device}")


def resolve(mode: str | None, mask: Any, n: int, h: int, w: int, device: Any) -> tuple[bool, torch.Tensor | None]:
    """(masked call?, explicit mask or None) for a call: the call's ``mask=`` (a tensor, or the name of a rule) wins over the normaliser's mode."""
    if isinstance(mask, str):
        check_mask_mode(mask)
        return True, None
    if mask is not None:
        check_mask_tensor(mask, n, h, w, device)
        return True, mask
    return mode is not None, None


def tissue_mask(images: torch.Tensor, luminosity_threshold: float = DEFAULT_LUMINOSITY_THRESHOLD, *, channel_axis: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """The luminosity rule on a batch: ``(mask, counts)`` -- ``mask`` (N, H, W) uint8, 1 = tissue, and ``counts`` (N,) int64 tissue pixels per
    tile, both on the device.  ``images``: NCHW (``channel_axis=-1``: NHWC) with C = 3, any supported element type; a CPU tensor is moved
    to the current GPU.  One streaming kernel (include/stainx_hip.h: sx_tissue_mask)."""
    threshold = check_threshold(luminosity_threshold)
    last = fe.image_4d(images, channel_axis, "tissue_mask")[0]
    from stainx_amd.backends.torch_hip_backend import tissue_mask_native

    return tissue_mask_native(images, threshold, last)


# ---------------------------------------------------------------------------------------------------------------- tissue detection
# A threshold taken from the data (Otsu on the lightness) and a morphological clean-up of the mask: what staintools', tiatoolbox's and
# HistomicsTK's users do on the CPU before an estimate.  The result is handed on as ``mask=det.mask``, which every masked call accepts.
MORPHOLOGY_OPS = ("erode", "dilate", "open", "close")
MORPHOLOGY_ELEMENTS = ("square", "disk")
MAX_MORPHOLOGY_RADIUS = 31      # include/stainx_hip.h: SX_MORPH_MAX_RADIUS
CONNECTIVITIES = (4, 8)         # 4: edge neighbours (scikit-image's connectivity=1); 8: diagonals too (connectivity=2, OpenCV's default)


class LuminosityHistogram(NamedTuple):
    """256-bin integer histograms of lightness (:func:`luminosity_histogram` returns it, :func:`otsu_threshold` takes it).  ``counts``: (rows,
    256) int64, ``pixels``: (rows,) int64, the row sums; both on the device.  rows = N for a histogram per tile, 1 pooled over a batch.
    Bin b holds the pixels that the luminosity rule calls tissue at threshold (b + 1) / 256 and not at b / 256 -- exactly: the bins are
    defined by the rule's own compare, so ``counts[:, :k].sum(1)`` IS ``tissue_mask(images, k / 256)[1]``.  Integers add up exactly:
    :meth:`pool` adds batches, slides or ranks into one row."""

    counts: torch.Tensor
    pixels: torch.Tensor

    @staticmethod
    def pool(*items: "LuminosityHistogram") -> "LuminosityHistogram":
        """One row, (1, 256) and (1,): the sum of every row of every argument (a torch add where the tensors live; exact)."""
        if not items:
            raise ValueError("pool needs at least one LuminosityHistogram")
        counts = pixels = None
        for item in items:
            c, p = _check_histogram(item)
            c, p = c.sum(dim=0, keepdim=True), p.sum(dim=0, keepdim=True)
            counts, pixels = (c, p) if counts is None else (counts + c, pixels + p)
        return LuminosityHistogram(counts, pixels)


class TissueDetection(NamedTuple):
    """What :func:`otsu_mask` returns: ``mask`` (N, H, W) uint8, 1 = tissue, and ``counts`` (N,) int64 tissue pixels per tile, both on the
    device; ``thresholds`` (N,) float64 on the CPU, the luminosity threshold each tile was cut at."""

    mask: torch.Tensor
    counts: torch.Tensor
    thresholds: torch.Tensor


class MaskComponents(NamedTuple):
    """What :func:`mask_components` returns, all on the device.  ``labels``: (N, H, W) int32 -- a set pixel holds ``1 + (y * W + x)`` of the first
    pixel of its component in raster order within its tile, an unset pixel 0: a function of the mask alone, the same on every run
    (``scipy.ndimage.label``, canonicalised).  ``areas``: (N, H, W) int32 -- at a component's first pixel its pixel count, 0 everywhere
    else (``areas[labels - 1]`` gathers a pixel's area; ``areas.flatten(1).topk(k)`` finds the k largest).  ``counts``: (N,) int64, the
    components per tile."""

    labels: torch.Tensor
    areas: torch.Tensor
    counts: torch.Tensor


def _check_histogram(hist: Any) -> tuple[torch.Tensor, torch.Tensor]:
    if not (isinstance(hist, (tuple, list)) and len(hist) == 2 and all(isinstance(t, torch.Tensor) for t in hist)):
        raise ValueError("expected a LuminosityHistogram (counts, pixels)")
    counts, pixels = hist
    if counts.dim() != 2 or counts.shape[1] != 256 or counts.shape[0] < 1:
        raise ValueError(f"histogram counts must have shape (rows, 256) with rows >= 1, got {tuple(counts.shape)}")
    if tuple(pixels.shape) != (counts.shape[0],):
        raise ValueError(f"histogram pixels must have shape (rows,) = ({counts.shape[0]},), got {tuple(pixels.shape)}")
    for name, value in (("counts", counts), ("pixels", pixels)):
        if value.dtype != torch.int64:
            raise ValueError(f"histogram {name} must have dtype int64, got {value.dtype}")
    return counts, pixels


def _check_radius(radius: Any, name: str, least: int) -> int:
    return fe.whole_number(radius, f"{name} must be an integer in {least}..{MAX_MORPHOLOGY_RADIUS}", least, MAX_MORPHOLOGY_RADIUS)


def _check_element(element: Any) -> str:
    if not isinstance(element, str) or element not in MORPHOLOGY_ELEMENTS:
        raise ValueError(f"element must be one of {list(MORPHOLOGY_ELEMENTS)}, got {element!r}")
    return element


def _check_area(area: Any, name: str, least: int) -> int:
    return fe.whole_number(area, f"{name} must be an integer of at least {least}", least)


def _check_connectivity(connectivity: Any) -> int:
    return fe.whole_number(connectivity, f"connectivity must be one of {list(CONNECTIVITIES)}", among=CONNECTIVITIES)


def _check_detection_mask(mask: Any) -> None:
    """A mask handed to the morphology calls: :func:`check_mask_tensor`'s rules with the mask's own sizes, and it has to live on a GPU."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a uint8 / bool tensor, got {type(mask).__name__}")
    if mask.dim() not in (3, 4) or (mask.dim() == 4 and mask.shape[1] != 1):
        raise ValueError(f"mask shape must be (N, H, W) or (N, 1, H, W), got {tuple(mask.shape)}")
    check_mask_tensor(mask, mask.shape[0], mask.shape[-2], mask.shape[-1], "cuda")


def luminosity_histogram(images: torch.Tensor, *, pooled: bool = False, channel_axis: int = 1) -> LuminosityHistogram:
    """256-bin integer histograms of lightness, per tile or (``pooled=True``) one for the batch: a memset and one streaming kernel
    (include/stainx_hip.h: sx_luminosity_histogram).  ``images`` as for :func:`tissue_mask`.  See :class:`LuminosityHistogram` for what a
    bin is; a NaN pixel lands in bin 255."""
    last = fe.image_4d(images, channel_axis, "luminosity_histogram")[0]
    from stainx_amd.backends.torch_hip_backend import luminosity_histogram_native

    counts = luminosity_histogram_native(images, bool(pooled), last)
    return LuminosityHistogram(counts, counts.sum(dim=1))


def otsu_threshold(hist: LuminosityHistogram, *, fallback: float = DEFAULT_LUMINOSITY_THRESHOLD) -> torch.Tensor:
    """Otsu's threshold of every row of ``hist``: float64 ``(rows,)`` on the CPU, each on the ``k / 256`` lattice (k = 1..255) -- what
    :func:`tissue_mask` takes as ``luminosity_threshold``: class 0, the tissue, is the bins below k.

    The between-class variance is computed over the bin indices from the integer counts in exact integer arithmetic on the host, so the
    call copies ``rows x 256`` integers from the device: THIS IS A SYNCHRONISATION POINT (and the only one of :func:`otsu_mask`).  Among
    the k that reach the exact maximum it takes ``(k_first + k_last) // 2``: between two separated modes every k of the gap is a
    maximiser, and the first would put the cut on the tissue mode's shoulder.  A row in which no k has both classes populated (one
    populated bin, or no pixels) gets ``fallback``.

    Known hazard: Otsu ALWAYS splits.  On a tile without glass it splits the tissue itself, on a tile of glass alone it splits the glass.
    Per-tile thresholds are for tiles that hold both; otherwise pool the histogram over the slide (:meth:`LuminosityHistogram.pool`,
    ``pooled=True``) or threshold a thumbnail."""
    counts, _ = _check_histogram(hist)
    fallback = check_threshold(fallback)
    out = []
    for row in counts.cpu().tolist():
        if any(c < 0 for c in row):
            raise ValueError("histogram counts must not be negative")
        total = sum(row)
        weighted = sum(i * c for i, c in enumerate(row))
        best_num, best_den, first, last = -1, 1, 0, 0
        n0 = s0 = 0
        for k in range(1, 256):
            n0 += row[k - 1]
            s0 += (k - 1) * row[k - 1]
            n1 = total - n0
            if n0 == 0 or n1 == 0:
                continue
            # w0 w1 (mu0 - mu1)^2 = (s0 n1 - s1 n0)^2 / (n0 n1 total^2): compared as fractions of integers
            num, den = (s0 * n1 - (weighted - s0) * n0) ** 2, n0 * n1
            side = num * best_den - best_num * den
            if best_num < 0 or side > 0:
                best_num, best_den, first, last = num, den, k, k
            elif side == 0:
                last = k
        out.append((first + last) // 2 / 256.0 if best_num >= 0 else fallback)
    return torch.tensor(out, dtype=torch.float64)


def mask_morphology(mask: torch.Tensor, op: str, radius: int, *, element: str = "disk") -> tuple[torch.Tensor, torch.Tensor]:
    """Binary morphology on a batch of masks: ``(mask, counts)`` -- (N, H, W) uint8, 1 / 0, and (N,) int64 set pixels per tile, on the device.
    ``mask``: (N, H, W) or (N, 1, H, W), uint8 or bool, on the GPU, non-zero = set.  ``op``: "erode", "dilate", "open" (erode, then dilate)
    or "close" (dilate, then erode); ``element``: "disk" (the offsets with dx^2 + dy^2 <= r^2, scikit-image's ``disk(r)``) or "square" (the
    (2r+1)^2 box); ``radius``: 1..31.  Borders as OpenCV's default and scipy's ``binary_erosion(border_value=1)`` /
    ``binary_dilation(border_value=0)``: what lies outside a tile never constrains the result, and tiles are independent.  One launch
    for erode / dilate, two for open / close (include/stainx_hip.h: sx_mask_morphology)."""
    if not isinstance(op, str) or op not in MORPHOLOGY_OPS:
        raise ValueError(f"op must be one of {list(MORPHOLOGY_OPS)}, got {op!r}")
    _check_radius(radius, "radius", 1)
    _check_element(element)
    _check_detection_mask(mask)
    from stainx_amd.backends.torch_hip_backend import mask_morphology_native

    return mask_morphology_native(mask, op, radius, element)


def mask_components(mask: torch.Tensor, *, connectivity: int = 8, holes: bool = False) -> MaskComponents:
    """Connected components of a batch of masks: :class:`MaskComponents` ``(labels, areas, counts)``.  ``mask`` as for :func:`mask_morphology`;
    tiles are independent: nothing outside a tile belongs to a component, and none continues into the next tile.  ``connectivity``: 4
    (edge neighbours: scipy's ``generate_binary_structure(2, 1)``, scikit-image's ``connectivity=1``) or 8 (diagonals too: ``np.ones((3, 3))``,
    ``connectivity=2``, OpenCV's default).  ``holes=True`` labels the components of the COMPLEMENT under the same connectivity -- a
    background region that touches the tile's edge is one of them.  Three launches, no synchronisation (include/stainx_hip.h:
    sx_mask_components)."""
    _check_connectivity(connectivity)
    _check_detection_mask(mask)
    from stainx_amd.backends.torch_hip_backend import mask_components_native

    return MaskComponents(*mask_components_native(mask, connectivity, bool(holes)))


def remove_small_objects(mask: torch.Tensor, min_area: int, *, connectivity: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """Clears every set pixel whose component has fewer than ``min_area`` pixels (an area equal to ``min_area`` stays): scikit-image's
    ``remove_small_objects``, tiatoolbox's ``min_region_size``.  Returns ``(mask, counts)`` as :func:`mask_morphology`; ``min_area=1`` gives the
    mask's own bits as 1 / 0, a value above H * W clears everything.  Components as in :func:`mask_components`.  No synchronisation
    (include/stainx_hip.h: sx_mask_area_filter)."""
    _check_area(min_area, "min_area", 1)
    _check_connectivity(connectivity)
    _check_detection_mask(mask)
    from stainx_amd.backends.torch_hip_backend import mask_area_filter_native

    return mask_area_filter_native(mask, min_area, connectivity, False)


def remove_small_holes(mask: torch.Tensor, min_area: int, *, connectivity: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """Sets every unset pixel whose component OF THE COMPLEMENT (same connectivity) has fewer than ``min_area`` pixels: scikit-image's
    ``remove_small_holes``.  Bit for bit ``1 - remove_small_objects(1 - mask, min_area)``.  Returns ``(mask, counts)`` as
    :func:`mask_morphology`; ``min_area=1`` gives the mask's own bits as 1 / 0, a value above H * W sets everything.

    Known hazard: a hole is ANY component of the complement -- a background region that touches the tile's edge counts as one.  On a
    tile whose glass is smaller than ``min_area`` THE GLASS IS FILLED.  Threshold a thumbnail, or choose ``min_area`` below a tile's glass."""
    _check_area(min_area, "min_area", 1)
    _check_connectivity(connectivity)
    _check_detection_mask(mask)
    from stainx_amd.backends.torch_hip_backend import mask_area_filter_native

    return mask_area_filter_native(mask, min_area, connectivity, True)


def refine_mask(mask: torch.Tensor, *, open_radius: int = 0, close_radius: int = 0, element: str = "disk", min_object_area: int = 0, min_hole_area: int = 0,
                connectivity: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """The clean-up of a tissue mask, in this order: objects below ``min_object_area`` pixels go (:func:`remove_small_objects`), an opening
    (specks of dust go) of ``open_radius``, a closing (holes go) of ``close_radius``, holes below ``min_hole_area`` pixels are filled
    (:func:`remove_small_holes`, whose hazard applies: glass smaller than ``min_hole_area`` is filled, edge-touching or not).  A radius or an
    area of 0 skips its step: filtering by area first lets the opening stay small, and filling last measures what the closing left.
    Returns ``(mask, counts)`` as :func:`mask_morphology`; with every step skipped, the mask's own bytes as 1 / 0."""
    _check_radius(open_radius, "open_radius", 0)
    _check_radius(close_radius, "close_radius", 0)
    _check_element(element)
    _check_area(min_object_area, "min_object_area", 0)
    _check_area(min_hole_area, "min_hole_area", 0)
    _check_connectivity(connectivity)
    _check_detection_mask(mask)
    out = mask[:, 0] if mask.dim() == 4 else mask
    counts = None
    if min_object_area:
        out, counts = remove_small_objects(out, min_object_area, connectivity=connectivity)
    if open_radius:
        out, counts = mask_morphology(out, "open", open_radius, element=element)
    if close_radius:
        out, counts = mask_morphology(out, "close", close_radius, element=element)
    if min_hole_area:
        out, counts = remove_small_holes(out, min_hole_area, connectivity=connectivity)
    if counts is None:
        out = (out != 0).to(torch.uint8)
        counts = out.sum(dim=(1, 2), dtype=torch.int64)
    return out, counts


def otsu_mask(images: torch.Tensor, *, pooled: bool = False, channel_axis: int = 1, fallback: float = DEFAULT_LUMINOSITY_THRESHOLD, open_radius: int = 0,
              close_radius: int = 0, element: str = "disk", min_object_area: int = 0, min_hole_area: int = 0, connectivity: int = 8) -> TissueDetection:
    """Tissue detection on a batch: the luminosity histogram, Otsu's threshold per tile (``pooled=True``: one for the batch, repeated), the
    rule at each tile's threshold (sx_tissue_mask_tiles), then :func:`refine_mask` with the radii and areas given (its order: small objects
    go, opening, closing, small holes are filled -- and its hazard: glass below ``min_hole_area`` is filled).  Without them tile i's mask has the bits of
    ``tissue_mask(images[i:i+1], thresholds[i])``.  One synchronisation point: :func:`otsu_threshold`, which also states the hazard --
    Otsu always splits, so per-tile thresholds are for tiles that hold both tissue and glass; otherwise pool, or threshold a thumbnail."""
    last = fe.image_4d(images, channel_axis, "otsu_mask")[0]
    fallback = check_threshold(fallback)
    _check_radius(open_radius, "open_radius", 0)
    _check_radius(close_radius, "close_radius", 0)
    _check_element(element)
    _check_area(min_object_area, "min_object_area", 0)
    _check_area(min_hole_area, "min_hole_area", 0)
    _check_connectivity(connectivity)
    from stainx_amd.backends.torch_hip_backend import tissue_mask_tiles_native

    thresholds = otsu_threshold(luminosity_histogram(images, pooled=pooled, channel_axis=channel_axis), fallback=fallback)
    if pooled:
        thresholds = thresholds.repeat(images.shape[0])
    mask, counts = tissue_mask_tiles_native(images, thresholds, last)
    if open_radius or close_radius or min_object_area or min_hole_area:
        mask, counts = refine_mask(mask, open_radius=open_radius, close_radius=close_radius, element=element, min_object_area=min_object_area,
                                   min_hole_area=min_hole_area, connectivity=connectivity)
    return TissueDetection(mask, counts, thresholds)


# ------------------------------------------------------------------------------------------------ saturation-channel tissue detection
# The front half of CLAM's segmentTissue: the HSV saturation as 8-bit levels, a median filter on it, a threshold (fixed, or Otsu on the
# level histogram), and the mask ``level > t``.  What follows the mask -- refine_mask, the area filters, every ``mask=`` -- takes it as it is.
MEDIAN_SIZES = (3, 5, 7, 9, 11, 13, 15)      # include/stainx_hip.h: odd, 3 .. SX_MEDIAN_MAX_SIZE
DEFAULT_SATURATION_FALLBACK = 8              # CLAM's sthresh


class LevelHistogram(NamedTuple):
    """256-bin integer histograms of a level map (:func:`level_histogram` returns it; :func:`otsu_level` and :func:`otsu_threshold` take it).
    ``counts``: (rows, 256) int64, bin b = the pixels of level b; ``pixels``: (rows,) int64, the row sums; both on the device.  rows = N for
    a histogram per tile, 1 pooled over a batch.  Integers add up exactly: :meth:`pool` adds batches, slides or ranks into one row."""

    counts: torch.Tensor
    pixels: torch.Tensor

    @staticmethod
    def pool(*items: "LevelHistogram") -> "LevelHistogram":
        """One row, (1, 256) and (1,): the sum of every row of every argument (a torch add where the tensors live; exact)."""
        if not items:
            raise ValueError("pool needs at least one LevelHistogram")
        return LevelHistogram(*LuminosityHistogram.pool(*items))


class SaturationDetection(NamedTuple):
    """What :func:`saturation_mask` returns: ``mask`` (N, H, W) uint8, 1 = tissue, and ``counts`` (N,) int64 tissue pixels per tile, both on the
    device; ``thresholds`` (N,) int64 on the CPU, the saturation level each tile was cut at (tissue iff level > threshold)."""

    mask: torch.Tensor
    counts: torch.Tensor
    thresholds: torch.Tensor


def _check_levels(levels: Any, what: str) -> None:
    """A level map: uint8 (a bool mask counts as 0 / 1), (N, H, W) or (N, 1, H, W), on a GPU."""
    if not isinstance(levels, torch.Tensor):
        raise ValueError(f"{what} expects a uint8 / bool tensor of levels, got {type(levels).__name__}")
    if levels.dim() not in (3, 4) or (levels.dim() == 4 and levels.shape[1] != 1):
        raise ValueError(f"levels shape must be (N, H, W) or (N, 1, H, W), got {tuple(levels.shape)}")
    if levels.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"levels dtype must be uint8 or bool, got {levels.dtype}")
    if levels.device.type != "cuda":
        raise ValueError(f"levels device must be a GPU, got {levels.device}")


def _check_median_size(size: Any, name: str = "size") -> int:
    return fe.whole_number(size, f"{name} must be an odd integer in 3..{MEDIAN_SIZES[-1]}", among=MEDIAN_SIZES)


def _check_level(level: Any, name: str) -> int:
    return fe.whole_number(level, f"{name} must be an integer level in 0..254", 0, 254)


def saturation_map(images: torch.Tensor, *, channel_axis: int = 1) -> torch.Tensor:
    """The HSV saturation of a batch as 8-bit levels: (N, H, W) uint8 on the device, one streaming kernel (include/stainx_hip.h:
    sx_saturation_map).  ``images`` as for :func:`tissue_mask`.

    The 8-bit level of a stored element: a uint8 is its own level; any other type gives ``rint(clip(255 * v, 0, 255))`` of its unit value
    in float32 (a double is rounded to float first; round-half-even; +inf is 255, -inf 0).  So a ``u / 255`` float32 or float64 tile has
    the levels, and the map, of its uint8 original.  So has an f16 or bf16 tile rounded from ``u / 255``, but bf16 only just: its
    rounding moves ``255 * v`` by up to 0.498 of a level, and any further arithmetic on a bf16 tile loses levels.  With M and m the largest and
    smallest of a pixel's three levels, ``S = 0`` if ``M == 0``, else ``(510 * (M - m) + M) // (2 * M)``: 255 (M - m) / M rounded half up, in
    0..255.  A pixel with a NaN in any channel has S = 0: background, as under the luminosity rule.  This is the package's own exact
    rule; it is not pinned to OpenCV's table-based conversion."""
    last = fe.image_4d(images, channel_axis, "saturation_map")[0]
    from stainx_amd.backends.torch_hip_backend import saturation_map_native

    return saturation_map_native(images, last)


def median_filter(levels: torch.Tensor, size: int) -> torch.Tensor:
    """The ``size x size`` median of a batch of level maps: (N, H, W) uint8 on the device, each the value of rank ``(size**2 + 1) // 2`` among
    the window centred on the pixel.  ``levels``: (N, H, W) or (N, 1, H, W) uint8 on the GPU; a bool mask is read as 0 / 1, on which the
    median is the majority filter.  ``size``: odd, 3..15.  The window is read with replicated borders inside the pixel's own tile
    (``cv2.medianBlur``'s border; bit for bit ``scipy.ndimage.median_filter(size=size, mode="nearest")``); tiles never see each other.
    One launch, no workspace, no synchronisation (include/stainx_hip.h: sx_median_filter_u8)."""
    _check_median_size(size)
    _check_levels(levels, "median_filter")
    from stainx_amd.backends.torch_hip_backend import median_filter_native

    return median_filter_native(levels, size)


def level_histogram(levels: torch.Tensor, *, pooled: bool = False) -> LevelHistogram:
    """256-bin integer histograms of level maps, per tile or (``pooled=True``) one for the batch: bin b counts the pixels of level b.  A
    memset and one launch (include/stainx_hip.h: sx_level_histogram).  ``levels`` as for :func:`median_filter`."""
    _check_levels(levels, "level_histogram")
    from stainx_amd.backends.torch_hip_backend import level_histogram_native

    counts = level_histogram_native(levels, bool(pooled))
    return LevelHistogram(counts, counts.sum(dim=1))


def otsu_level(hist: LevelHistogram, *, fallback: int = DEFAULT_SATURATION_FALLBACK) -> torch.Tensor:
    """Otsu's threshold of every row of a level histogram as a LEVEL: int64 ``(rows,)`` on the CPU, what :func:`level_mask` takes.  It is
    ``256 * otsu_threshold(hist, fallback=(fallback + 1) / 256) - 1``: class 0, the background, is the levels <= t (cv2's Otsu convention) and
    tissue is ``level > t``.  ``fallback``: 0..254, the level of a row with no split (one populated bin, or no pixels); 8 is CLAM's ``sthresh``.

    It inherits everything :func:`otsu_threshold` states: the synchronisation point, the plateau rule (among the exact maximisers the
    middle of the first and the last, so two separated modes are cut in the middle of the gap) and the hazard -- Otsu ALWAYS splits: a
    tile of tissue alone, or of glass alone, is split all the same.  Pool the histogram (:meth:`LevelHistogram.pool`, ``pooled=True``), or
    use a fixed level, where tiles do not hold both."""
    fallback = _check_level(fallback, "fallback")
    cut = otsu_threshold(hist, fallback=(fallback + 1) / 256.0)
    return (cut * 256.0).round().to(torch.int64) - 1


def level_mask(levels: torch.Tensor, thresholds: Any) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mask, counts)``: (N, H, W) uint8, tile i set where ``level > thresholds[i]`` (cv2's ``THRESH_BINARY``, CLAM's ``sthresh``), and (N,) int64 set
    pixels per tile, on the device.  ``thresholds``: an int (every tile), or an (N,) integer tensor on either device; a negative threshold
    sets the whole tile, one >= 255 clears it.  The kernel reads the thresholds from device memory: nothing here synchronises, and a
    captured call replayed after new thresholds were written into a device tensor uses them.  One launch and the clear of the counts
    (include/stainx_hip.h: sx_level_mask_tiles).  ``levels`` as for :func:`median_filter`."""
    _check_levels(levels, "level_mask")
    n = levels.shape[0]
    if isinstance(thresholds, torch.Tensor):
        if thresholds.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) or tuple(thresholds.shape) != (n,):
            raise ValueError(f"thresholds must be an int or an integer tensor of shape ({n},), got {thresholds.dtype} {tuple(thresholds.shape)}")
        cuts = thresholds.to(torch.int64).clamp(-1, 255).to(device=levels.device, dtype=torch.int32).contiguous()      # (widened first: -1 is no uint8)
    elif isinstance(thresholds, int) and not isinstance(thresholds, bool):
        cuts = torch.full((n,), min(max(thresholds, -1), 255), dtype=torch.int32, device=levels.device)
    else:
        raise ValueError(f"thresholds must be an int or an integer tensor of shape ({n},), got {type(thresholds).__name__}")
    from stainx_amd.backends.torch_hip_backend import level_mask_native

    return level_mask_native(levels, cuts)


def saturation_mask(images: torch.Tensor, *, threshold: int | None = None, median_size: int = 7, pooled: bool = False, channel_axis: int = 1,
                    fallback: int = DEFAULT_SATURATION_FALLBACK, open_radius: int = 0, close_radius: int = 0, element: str = "disk", min_object_area: int = 0,
                    min_hole_area: int = 0, connectivity: int = 8) -> SaturationDetection:
    """Tissue detection on the saturation channel (the front half of CLAM's ``segmentTissue``), in this order: :func:`saturation_map`; the
    :func:`median_filter` of ``median_size`` (0 skips it); the threshold; :func:`level_mask`; then :func:`refine_mask` with the radii and areas
    given, when any is non-zero.  ``threshold=None``: Otsu by :func:`level_histogram` and :func:`otsu_level`, per tile or (``pooled=True``) one for
    the batch, repeated -- the one synchronisation point.  ``threshold`` an integer in 0..254: that level for every tile; this path does
    not synchronise and can be captured in a graph.  CLAM's defaults are ``saturation_mask(x, threshold=8, median_size=7, close_radius=4,
    element="square")`` followed by the area filters.

    Known hazards.  Near-black pixels have an unstable, often high, saturation -- (10, 10, 12) has S = 43 -- so BLACK MARKER PASSES this
    rule, as it does in CLAM: AND the result with :func:`tissue_mask` where that matters.  COLOURED PEN is saturated and passes too.  And
    with ``threshold=None`` Otsu ALWAYS splits (:func:`otsu_level`): per-tile thresholds are for tiles that hold both tissue and glass."""
    fe.image_4d(images, channel_axis, "saturation_mask")
    if threshold is not None:
        _check_level(threshold, "threshold")
    if isinstance(median_size, bool) or not isinstance(median_size, int) or median_size != 0:
        _check_median_size(median_size, "median_size")
    fallback = _check_level(fallback, "fallback")
    _check_radius(open_radius, "open_radius", 0)
    _check_radius(close_radius, "close_radius", 0)
    _check_element(element)
    _check_area(min_object_area, "min_object_area", 0)
    _check_area(min_hole_area, "min_hole_area", 0)
    _check_connectivity(connectivity)
    levels = saturation_map(images, channel_axis=channel_axis)
    if median_size:
        levels = median_filter(levels, median_size)
    n = levels.shape[0]
    if threshold is None:
        thresholds = otsu_level(level_histogram(levels, pooled=pooled), fallback=fallback)
        if pooled:
            thresholds = thresholds.repeat(n)
        mask, counts = level_mask(levels, thresholds)
    else:
        thresholds = torch.full((n,), threshold, dtype=torch.int64)
        mask, counts = level_mask(levels, threshold)
    if open_radius or close_radius or min_object_area or min_hole_area:
        mask, counts = refine_mask(mask, open_radius=open_radius, close_radius=close_radius, element=element, min_object_area=min_object_area,
                                   min_hole_area=min_hole_area, connectivity=connectivity)
    return SaturationDetection(mask, counts, thresholds)
