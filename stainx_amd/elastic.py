"""Elastic deformation: a control grid per tile under a cubic B-spline, fused with the affine warp in one launch (an extension: the
reference has none).

The other half of the "morphology" set of Tellez et al. 2019 (the paper ``AffineAugment`` cites).  A smooth displacement field needs no
dense flow: every tile has a small grid of control displacements ``(2, GH, GW)`` float32 -- plane 0 ``dx``, plane 1 ``dy``, in SOURCE
pixels, one control point every ``cell`` OUTPUT pixels --, read on the device and evaluated on chip; the displacement is added to the
affine coordinate of ``affine_warp`` and everything else is that call's rule.  ``elastic_warp`` is one launch per batch
(include/stainx_hip.h: sx_elastic_warp), ``elastic_warp_mask`` warps a mask WITH its tile, ``elastic_grids`` draws grids on the device,
``simard_parameters`` maps Simard's ``(alpha, sigma)`` onto ``(cell, magnitude)`` and ``ElasticAugment`` is the ``nn.Module`` beside
``AffineAugment`` -- with ``affine=`` the whole morphology set and the crop in ONE launch.

The rule: ``GH = (OH - 1) // cell + 4`` and ``GW`` likewise; control column ``j`` sits at output column ``(j - 1) cell``.  For output
pixel ``(x, y)``: ``jx = x // cell``, ``tx = (x - jx cell) / cell``, ``jy``, ``ty`` likewise, and with the uniform cubic B-spline weights
``B0 = (1 - t)^3 / 6``, ``B1 = (3 t^3 - 6 t^2 + 4) / 6``, ``B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6``, ``B3 = t^3 / 6``:
``dx = sum_l B_l(ty) sum_k B_k(tx) P0[jy + l][jx + k]``, ``dy`` from plane 1; ``sx = a x + b y + c + dx``, ``sy = d x + e y + f + dy``.
A zero grid gives ``affine_warp``'s result bit for bit; a NaN, an infinite or a huge displacement gives ``fill``; a row with a NaN or an
infinity leaves its tile (copy, centre crop or centre pad) and its grid is not read.
"""
from __future__ import annotations

import math
from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe
from stainx_amd.warp import BORDERS, INTERPOLATIONS, AffineAugment, _check_choice, _check_fill, _check_fill_byte, _check_mask, _check_out_dtype, _check_rows, _check_size, _per_tile, _range

MIN_CELL, MAX_CELL = 4, 4096      # include/stainx_hip.h: SX_ELASTIC_MIN_CELL, SX_ELASTIC_MAX_CELL
SPLINE_STD = 151.0 / 315.0        # the standard deviation of the spline field of unit control displacements (``simard_parameters``)
_ENGINES: dict[torch.device, Any] = {}
_ANCHORS: dict[tuple, torch.Tensor] = {}      # (device, H, W, OH, OW) -> the (1, 6) anchor row, uploaded once: a host copy per call would keep a call from being captured


# ------------------------------------------------------------------------------------------------------------------ the checks
def _check_cell(cell: Any) -> int:
    return fe.whole_number(cell, f"cell must be an int in {MIN_CELL}..{MAX_CELL} (the control spacing in output pixels)", MIN_CELL, MAX_CELL)


def elastic_grid_shape(size: tuple[int, int], cell: int) -> tuple[int, int]:
    """``(GH, GW)`` of the control grid for an output of ``size = (OH, OW)``: ``(OH - 1) // cell + 4`` and ``(OW - 1) // cell + 4`` --
    one control point left of (above) the first pixel's cell and two past the last pixel's."""
    checked = _check_size(size)
    if checked is None:
        raise ValueError("size must be an (OH, OW) pair of positive ints, got None")
    cell = _check_cell(cell)
    return (checked[0] - 1) // cell + 4, (checked[1] - 1) // cell + 4


def _check_grids(grids: Any, n: int, size: tuple[int, int], cell: int) -> None:
    """Checked by shape only: the values live on the device."""
    gh, gw = elastic_grid_shape(size, cell)
    shape = tuple(getattr(grids, "shape", ()))
    if not isinstance(grids, torch.Tensor) or not (shape == (2, gh, gw) or (len(shape) == 4 and shape[1:] == (2, gh, gw) and shape[0] in (1, n))):
        raise ValueError(f"grids must be a tensor of shape (2, GH, GW), (1, 2, GH, GW) or (N, 2, GH, GW) = ({n}, 2, {gh}, {gw}) for a {size[0]} x {size[1]} output at cell {cell}, "
                         f"got {shape if isinstance(grids, torch.Tensor) else type(grids).__name__}")


def anchor_rows(in_size: tuple[int, int], out_size: tuple[int, int], device: torch.device) -> torch.Tensor:
    """The (1, 6) row ``(1, 0, (W - OW) // 2, 0, 1, (H - OH) // 2)`` on ``device``: the row a tile that is left uses -- the identity
    where the sizes are equal, else the centre crop or pad.  Kept per device and sizes."""
    device = torch.device(device)
    key = (device, *in_size, *out_size)
    row = _ANCHORS.get(key)
    if row is None:
        row = _ANCHORS[key] = torch.tensor([[1.0, 0.0, (in_size[1] - out_size[1]) // 2, 0.0, 1.0, (in_size[0] - out_size[0]) // 2]], dtype=torch.float32, device=device)
    return row


# ------------------------------------------------------------------------------------------------------------------ the calls
def _elastic(images: torch.Tensor, grids: Any, rows: Any, who: str, *, cell: Any, size: Any, interpolation: str, border: str, fill: Any, channels_last: bool,
             normalize_to_0_1: bool, out_dtype: torch.dtype | None, device: torch.device | None, mask: Any = None) -> Any:
    """The one path of the entry points; every argument error is raised before any GPU work.  With ``mask``: ``(tiles, warped mask)``."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    cell = _check_cell(cell)
    size = _check_size(size) or (dims[1], dims[2])
    _check_grids(grids, dims[0], size, cell)
    if rows is not None:
        _check_rows(rows, dims[0])
    _check_choice("interpolation", interpolation, INTERPOLATIONS)
    _check_choice("border", border, BORDERS)
    fill = _check_fill(fill)
    _check_out_dtype(batch, out_dtype)
    flat_mask = single and isinstance(mask, torch.Tensor) and mask.dim() == 2      # (the (H, W) mask of a CHW tile comes back as (OH, OW))
    if mask is not None:
        if flat_mask:
            mask = mask.unsqueeze(0)
        if _check_mask(mask, who) != dims:
            raise ValueError(f"mask shape must be (N, H, W) or (N, 1, H, W) = {dims}, got {tuple(mask.shape)}")
    run_on = fe.run_device(device, batch.device, who)
    if rows is None:
        rows = anchor_rows(dims[1:], size, run_on)
    engine = fe.held(_ENGINES, run_on, fe.engine, "ElasticHIP")
    out = engine.apply(batch, rows, grids, cell, size, interpolation=interpolation, border=border, fill=fill, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype,
                       channels_last=channels_last)
    out = out.squeeze(0) if single else out
    if mask is None:
        return out
    warped = _elastic_mask(mask, grids, rows, engine, cell, size, border, 0)      # (the same rows and grids: the second launch)
    return out, (warped.squeeze(0) if flat_mask else warped)


def _elastic_mask(mask: torch.Tensor, grids: torch.Tensor, rows: torch.Tensor, engine: Any, cell: int, size: tuple[int, int], border: str, fill: int) -> torch.Tensor:
    out = engine.apply_mask(mask, rows, grids, cell, size, border=border, fill=fill)
    if mask.dim() == 4:
        out = out.unsqueeze(1)
    return out.view(torch.bool) if mask.dtype == torch.bool else out


def elastic_warp(images: torch.Tensor, grids: torch.Tensor, *, cell: int, rows: torch.Tensor | None = None, size: tuple[int, int] | None = None, interpolation: str = "bilinear",
                 border: str = "mirror", fill: float = 0.0, channel_axis: int = 1, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """The functional form: ``grids`` a tensor of shape (2, GH, GW), (1, 2, GH, GW) or (N, 2, GH, GW) with ``(GH, GW) =
    elastic_grid_shape(size, cell)`` -- control displacements in source pixels, plane 0 ``dx``, plane 1 ``dy``, read on the device, checked
    by shape only -- applied to CHW / NCHW tiles (``channel_axis=-1``: HWC / NHWC) on the GPU the tiles are on.  ``cell``: the control
    spacing in output pixels, an int in 4..4096.  ``rows``: affine rows as ``affine_warp`` takes them, in the same launch; ``None``: the
    anchor row (the identity, or the centre crop / pad to ``size``).  ``size``, ``interpolation``, ``border``, ``fill``,
    ``normalize_to_0_1`` and ``out_dtype`` as ``affine_warp``.  One launch, no synchronisation; the result never aliases the input."""
    return _elastic(images, grids, rows, "elastic_warp", cell=cell, size=size, interpolation=interpolation, border=border, fill=fill, channels_last=fe.channels_last(channel_axis),
                    normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


def elastic_warp_mask(mask: torch.Tensor, grids: torch.Tensor, *, cell: int, rows: torch.Tensor | None = None, size: tuple[int, int] | None = None, border: str = "constant",
                      fill: int = 0) -> torch.Tensor:
    """A mask warped WITH its tile: uint8 or bool, (N, H, W) or (N, 1, H, W) -> the same kind and rank at ``size``.  Nearest, bytes moved
    as bytes (labels 0..255 survive); the same ``grids``, ``cell`` and ``rows`` as the tiles' ``elastic_warp`` give the same coordinates:
    the nearest warp of an image and the warp of its mask stay aligned."""
    n, h, w = _check_mask(mask, "elastic_warp_mask")
    cell = _check_cell(cell)
    size = _check_size(size) or (h, w)
    _check_grids(grids, n, size, cell)
    if rows is not None:
        _check_rows(rows, n)
    _check_choice("border", border, BORDERS)
    fill = _check_fill_byte(fill)
    run_on = fe.run_device(None, mask.device, "elastic_warp_mask")
    if rows is None:
        rows = anchor_rows((h, w), size, run_on)
    return _elastic_mask(mask, grids, rows, fe.held(_ENGINES, run_on, fe.engine, "ElasticHIP"), cell, size, border, fill)


# ------------------------------------------------------------------------------------------------------------------ the grids
def elastic_grids(n: int, size: tuple[int, int], cell: int, magnitude: Any, *, generator: torch.Generator | None = None, device: str | torch.device | None = None) -> torch.Tensor:
    """(N, 2, GH, GW) float32 control grids on ``device`` (default: the generator's, else the CPU) for an output of ``size = (OH, OW)``:
    ONE draw, ``randn((n, 2, GH, GW))`` with ``generator`` on the generator's device -- tile by tile, plane ``dx`` before plane ``dy``,
    row by row --, times ``magnitude``: the standard deviation of the control displacements in source pixels, a number >= 0 or an ``(N,)``
    tensor (checked by shape only).  With a generator ON the device nothing is copied from the host."""
    n = fe.whole_number(n, "n must be a positive int", lo=1)
    gh, gw = elastic_grid_shape(size, cell)
    device = torch.device(device) if device is not None else (generator.device if generator is not None else torch.device("cpu"))
    scale = _per_tile(magnitude, n, "magnitude", device, lambda v: math.isfinite(v) and v >= 0.0, "must be finite and >= 0").to(torch.float32)
    return fe.draw(generator, (n, 2, gh, gw), device, "randn").to(device) * scale.view(n, 1, 1, 1)


def simard_parameters(alpha: float, sigma: float) -> tuple[int, float]:
    """``(cell, magnitude)`` for ``elastic_grids`` from the parametrisation of Simard et al. 2003, which Tellez et al. use: the field
    ``alpha * gaussian_filter(U(-1, 1), sigma)`` per axis.

    Smoothness.  The uniform cubic B-spline of spacing ``cell`` is, as a smoothing kernel, the four-fold convolution of a box of width
    ``cell``: its variance is ``4 * cell^2 / 12 = cell^2 / 3``.  Equal to the Gaussian's ``sigma^2``: ``cell = sqrt(3) sigma``, rounded
    to an int and kept within 4..4096.

    Amplitude.  ``U(-1, 1)`` has variance 1/3; a filter of weights ``g`` multiplies the variance of white noise by ``sum g^2``, which
    for a 2-D Gaussian is ``1 / (4 pi sigma^2)``: the Simard field's standard deviation is ``alpha / (sqrt(3) * 2 sqrt(pi) * sigma)``.
    The spline field of control displacements of standard deviation ``magnitude`` has, at a pixel, the variance ``magnitude^2 *
    sum_k B_k(tx)^2 * sum_l B_l(ty)^2``; the mean over ``t`` of ``sum_k B_k(t)^2`` is ``151 / 315`` (it runs from 0.4603 at t = 1/2 to
    0.5 at t = 0), so the field's standard deviation is ``magnitude * 151 / 315`` (root-mean-square over the tile).  Equal:
    ``magnitude = alpha / (sqrt(3) * 2 sqrt(pi) * sigma) * 315 / 151``."""
    alpha = fe.real_number(alpha, "alpha must be a number", "alpha must be finite and >= 0", lambda v: math.isfinite(v) and v >= 0.0)
    sigma = fe.real_number(sigma, "sigma must be a number", "sigma must be finite and positive", lambda v: math.isfinite(v) and v > 0.0)
    cell = min(MAX_CELL, max(MIN_CELL, int(round(math.sqrt(3.0) * sigma))))
    return cell, alpha / (math.sqrt(3.0) * 2.0 * math.sqrt(math.pi) * sigma) / SPLINE_STD


# ----------------------------------------------------------------------------------------------------------------- the module
class ElasticAugment(nn.Module):
    """Random per-tile elastic deformation of CHW / NCHW tensors on an MI355X, one launch per batch.  Per tile the control displacements
    are normal with a standard deviation drawn uniformly from ``magnitude=(lo, hi)`` source pixels, one control point every ``cell``
    output pixels (``simard_parameters`` maps Simard's ``(alpha, sigma)`` onto the pair).  ``affine``: an ``AffineAugment`` whose
    ``sample_rows`` supplies the tiles' affine rows and whose ``size`` is the result's size -- rotation, scale, shear, the elastic
    deformation and the crop in ONE launch; its interpolation, border and fill are not used, this module's are.  With probability
    ``1 - p`` a tile gets a ZERO grid: it is then ``affine``'s warp of it, bit for bit (and, where ``affine`` leaves it too or there is
    none, a copy or the centre crop).  ``size`` (without ``affine``), ``interpolation``, ``border``, ``fill``, ``normalize_to_0_1``
    (default True), ``generator`` and ``device`` as ``AffineAugment``.  With a generator ON the device everything is drawn and built
    there: nothing is synchronised and a call is capturable."""

    def __init__(self, magnitude: tuple[float, float] = (0.0, 2.0), cell: int = 16, *, affine: AffineAugment | None = None, p: float = 1.0, size: tuple[int, int] | None = None,
                 interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0, normalize_to_0_1: bool = True, generator: torch.Generator | None = None,
                 device: str | torch.device | None = None):
        super().__init__()
        self.magnitude = _range("magnitude", magnitude, lambda v: math.isfinite(v) and v >= 0.0, "finite and >= 0")
        self.cell = _check_cell(cell)
        if affine is not None and not isinstance(affine, AffineAugment):
            raise ValueError(f"affine must be None or an AffineAugment, got {type(affine).__name__}")
        self.affine = affine
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        size = _check_size(size)
        if affine is not None and size is not None and size != affine.size:
            raise ValueError(f"size comes from affine= where one is given (affine.size = {affine.size}), got size={size}")
        self.size = affine.size if affine is not None else size
        self.interpolation = _check_choice("interpolation", interpolation, INTERPOLATIONS)
        self.border = _check_choice("border", border, BORDERS)
        self.fill = _check_fill(fill)
        self.device = fe.cuda_only(device, "ElasticAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator

    def sample(self, n: int, in_size: tuple[int, int], device: str | torch.device | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(rows, grids)``: (n, 6) and (n, 2, GH, GW) float32 on ``device`` for tiles of ``in_size = (H, W)``.  The draws, always and in
        this order: ``affine.sample_rows(n, in_size)`` where there is an ``affine`` (ITS draws, with ITS generator); ``rand(n)`` -- the
        tiles' magnitudes ``lo + (hi - lo) u`` --; ``elastic_grids``' one ``randn((n, 2, GH, GW))``; ``p < 1``: one more, ``rand(n) < p``.
        A tile that is not chosen gets a zero grid and keeps ``affine``'s row (a NaN row without ``affine``); a tile that is chosen keeps
        ``affine``'s row where that is finite and gets the anchor row where it is not (and without ``affine``)."""
        device = fe.draw_device(device, self.device)
        h, w = _check_size(in_size, "in_size")
        size = self.size or (h, w)
        given = self.affine.sample_rows(n, (h, w), device) if self.affine is not None else None
        u = fe.draw(self.generator, (n,), device).to(device)
        grids = elastic_grids(n, size, self.cell, self.magnitude[0] + (self.magnitude[1] - self.magnitude[0]) * u, generator=self.generator, device=device)
        chosen = fe.chosen(self.generator, n, self.p, device) if self.p < 1.0 else torch.ones((n, 1), dtype=torch.bool, device=device)
        grids = torch.where(chosen.view(n, 1, 1, 1), grids, torch.zeros_like(grids))
        anchor = anchor_rows((h, w), size, device).expand(n, 6)
        if given is None:
            rows = torch.where(chosen, anchor, torch.full_like(anchor, float("nan")))
        else:
            rows = torch.where(chosen & ~torch.isfinite(given).all(dim=1, keepdim=True), anchor, given)
        return rows, grids

    def forward(self, img: torch.Tensor, grids: torch.Tensor | None = None, rows: torch.Tensor | None = None, mask: Any = None) -> Any:
        """``grids`` and ``rows``: explicit ones instead of a draw (``grids`` alone: the anchor row; ``rows`` alone is refused -- the
        draw makes both).  ``mask``: a uint8 / bool tensor (N, H, W) or (N, 1, H, W) that is warped WITH the tiles (nearest, the module's
        border, 0 outside): the result is ``(tiles, warped mask)`` -- two launches, the same rows and grids."""
        if grids is None:
            if rows is not None:
                raise ValueError("rows= goes with grids=: without grids the module draws both")
            batch, _, (n, h, w) = fe.image_batch(img, False, "ElasticAugment")
            rows, grids = self.sample(n, (h, w), fe.run_device(self.device, batch.device, "ElasticAugment"))
        return _elastic(img, grids, rows, "ElasticAugment", cell=self.cell, size=self.size, interpolation=self.interpolation, border=self.border, fill=self.fill, channels_last=False,
                        normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device, mask=mask)

    def extra_repr(self) -> str:
        return (f"magnitude={self.magnitude}, cell={self.cell}, affine={'None' if self.affine is None else 'AffineAugment(...)'}, p={self.p}, size={self.size}, "
                f"interpolation={self.interpolation!r}, border={self.border!r}, fill={self.fill}, normalize_to_0_1={self.normalize_to_0_1}")
