"""Geometric augmentation: an affine map per tile, one launch (an extension: the reference has none).

The geometric half of Tellez et al. 2019's augmentation set (the paper ``HEDAugment``, ``HSVAugment`` and ``GaussianBlurAugment`` cite):
quarter turns and flips ("basic"), rotation, scaling, shear and translation ("morphology") -- and, in the same launch, the crop of a tile
out of a larger one and the resampling to another size.  Every tile has ONE row of six float32 ``(a, b, c, d, e, f)``; ``affine_warp`` is
one launch per batch (include/stainx_hip.h: sx_affine_warp) with the rows in device memory, ``affine_warp_mask`` warps a mask WITH its
tile (nearest, bytes moved as bytes), ``affine_rows`` builds rows on the device and ``AffineAugment`` is the ``nn.Module`` beside
``GaussianBlurAugment``.

The rule: a row maps an OUTPUT pixel ``(x, y)`` (column, row) to the SOURCE position ``sx = a x + b y + c``, ``sy = d x + e y + f`` in
pixel-index coordinates with pixel centres at integers (``scipy.ndimage.affine_transform``, ``cv2.warpAffine`` with ``WARP_INVERSE_MAP``,
``grid_sample(align_corners=True)`` un-normalised), float32 fused multiply-adds.  ``bilinear`` takes the four neighbours, ``nearest`` the
element at ``floor(s + 0.5)``; ``border="mirror"`` reflects without repeating the edge (scipy's ``mirror``, torch's ``reflection``),
``"constant"`` takes ``fill`` outside the tile (scipy's ``grid-constant``).  uint8 results are ROUNDED to the nearest level.  A row with a
NaN or an infinity means "leave this tile": a copy, bit for bit, where the sizes are equal, else the centre crop or the centre pad.  A
coordinate that is not finite or beyond ``MAX_COORD`` = 2^22 gives ``fill``.
"""
from __future__ import annotations

import math
from typing import Any

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe

MAX_COORD = 4194304.0      # include/stainx_hip.h: SX_WARP_MAX_COORD
INTERPOLATIONS = ("nearest", "bilinear")
BORDERS = ("mirror", "constant")
_ENGINES: dict[torch.device, Any] = {}      # (one engine per device for the module: the functional forms have no object to keep it)


# ------------------------------------------------------------------------------------------------------------------ the checks
def _check_rows(rows: Any, n: int) -> None:
    """Checked by shape only: the values live on the device."""
    shape = tuple(getattr(rows, "shape", ()))
    if not isinstance(rows, torch.Tensor) or not (shape == (6,) or (len(shape) == 2 and shape[1] == 6 and shape[0] in (1, n))):
        raise ValueError(f"rows must be a tensor of shape (6,), (1, 6) or (N, 6) = ({n}, 6) holding (a, b, c, d, e, f), got {shape if isinstance(rows, torch.Tensor) else type(rows).__name__}")


def _check_size(size: Any, name: str = "size") -> tuple[int, int] | None:
    if size is None:
        return None
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"{name} must be None or an (OH, OW) pair of positive ints, got {size!r}")
    return (fe.whole_number(size[0], f"{name} must be None or an (OH, OW) pair of positive ints", lo=1), fe.whole_number(size[1], f"{name} must be None or an (OH, OW) pair of positive ints", lo=1))


def _check_choice(name: str, value: Any, among: tuple) -> str:
    if value not in among:
        raise ValueError(f"{name} must be one of {among}, got {value!r}")
    return value


def _check_fill(fill: Any) -> float:
    return fe.real_number(fill, "fill must be a number", "fill must be finite", math.isfinite)


def _check_fill_byte(fill: Any) -> int:
    return fe.whole_number(fill, "fill must be an int in 0..255 (a mask's byte)", 0, 255)


def _check_out_dtype(images: torch.Tensor, out_dtype: Any) -> None:
    if out_dtype is not None and out_dtype != images.dtype and (images.dtype != torch.uint8 or out_dtype not in (torch.bfloat16, torch.float16)):
        raise ValueError(f"out_dtype is supported for uint8 input and bfloat16 / float16 output, got {images.dtype} -> {out_dtype}")


def _check_mask(mask: Any, who: str) -> tuple[int, int, int]:
    """A mask that is warped: uint8 / bool, (N, H, W) or (N, 1, H, W).  -> (n, h, w)"""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{who} expects a tensor, got {type(mask).__name__}")
    shape = tuple(mask.shape)
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask dtype must be uint8 or bool, got {mask.dtype}")
    if not (len(shape) == 3 or (len(shape) == 4 and shape[1] == 1)):
        raise ValueError(f"mask shape must be (N, H, W) or (N, 1, H, W), got {shape}")
    return shape[0], shape[-2], shape[-1]


# ------------------------------------------------------------------------------------------------------------------ the calls
def _warp(images: torch.Tensor, rows: Any, who: str, *, size: Any, interpolation: str, border: str, fill: Any, channels_last: bool, normalize_to_0_1: bool,
          out_dtype: torch.dtype | None, device: torch.device | None, mask: Any = None) -> Any:
    """The one path of the entry points; every argument error is raised before any GPU work.  With ``mask``: ``(tiles, warped mask)``."""
    batch, single, dims = fe.image_batch(images, channels_last, who)
    _check_rows(rows, dims[0])
    size = _check_size(size)
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
    engine = fe.held(_ENGINES, run_on, fe.engine, "WarpHIP")
    out = engine.apply(batch, rows, size, interpolation=interpolation, border=border, fill=fill, normalize_to_0_1=normalize_to_0_1, out_dtype=out_dtype, channels_last=channels_last)
    out = out.squeeze(0) if single else out
    if mask is None:
        return out
    warped = _warp_mask(mask, rows, engine, size, border, 0)      # (the same rows: the second launch)
    return out, (warped.squeeze(0) if flat_mask else warped)


def _warp_mask(mask: torch.Tensor, rows: Any, engine: Any, size: tuple[int, int] | None, border: str, fill: int) -> torch.Tensor:
    out = engine.apply_mask(mask, rows, size, border=border, fill=fill)
    if mask.dim() == 4:
        out = out.unsqueeze(1)
    return out.view(torch.bool) if mask.dtype == torch.bool else out


def affine_warp(images: torch.Tensor, rows: torch.Tensor, *, size: tuple[int, int] | None = None, interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0,
                channel_axis: int = 1, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """The functional form: ``rows`` a tensor of shape (6,), (1, 6) or (N, 6) -- a row ``(a, b, c, d, e, f)`` per tile, read on the device,
    checked by shape only -- applied to CHW / NCHW tiles (``channel_axis=-1``: HWC / NHWC) on the GPU the tiles are on.  ``size=(OH, OW)``:
    the result's size, default the input's -- crop, pad and resize are this call.  ``interpolation``: ``"bilinear"`` or ``"nearest"``;
    ``border``: ``"mirror"`` or ``"constant"`` with ``fill`` on the element's own scale (a level 0..255 for uint8 tiles).
    ``normalize_to_0_1``: uint8 tiles come out as float32 in [0, 1], float tiles are divided by 255; ``out_dtype``: bfloat16 / float16
    written directly from uint8 tiles.  A CHW tile gives a CHW tile.  One launch, no synchronisation; the result never aliases the input."""
    return _warp(images, rows, "affine_warp", size=size, interpolation=interpolation, border=border, fill=fill, channels_last=fe.channels_last(channel_axis),
                 normalize_to_0_1=bool(normalize_to_0_1), out_dtype=out_dtype, device=None)


def affine_warp_mask(mask: torch.Tensor, rows: torch.Tensor, *, size: tuple[int, int] | None = None, border: str = "constant", fill: int = 0) -> torch.Tensor:
    """A mask warped WITH its tile: uint8 or bool, (N, H, W) or (N, 1, H, W) -> the same kind and rank at ``size``.  Nearest, bytes moved
    as bytes (labels 0..255 survive); ``border="constant"`` takes the byte ``fill`` outside the tile, ``"mirror"`` reflects.  The same
    ``rows`` as the tiles' ``affine_warp``: the nearest warp of an image and the warp of its mask stay aligned."""
    n, _, _ = _check_mask(mask, "affine_warp_mask")
    _check_rows(rows, n)
    size = _check_size(size)
    _check_choice("border", border, BORDERS)
    fill = _check_fill_byte(fill)
    run_on = fe.run_device(None, mask.device, "affine_warp_mask")
    return _warp_mask(mask, rows, fe.held(_ENGINES, run_on, fe.engine, "WarpHIP"), size, border, fill)


# ------------------------------------------------------------------------------------------------------------------- the rows
def _per_tile(value: Any, n: int, name: str, device: torch.device, accepts=math.isfinite, rule: str = "must be finite") -> torch.Tensor:
    """A number (checked) or a tensor of shape () or (N,) (checked by shape only) -> (N,) float64 on ``device``."""
    if isinstance(value, torch.Tensor):
        if tuple(value.shape) not in ((), (n,)):
            raise ValueError(f"{name} must be a number or a tensor of shape () or (N,) = ({n},), got {tuple(value.shape)}")
        return value.to(device=device, dtype=torch.float64).expand(n)
    number = fe.real_number(value, f"{name} must be a number or a tensor", f"{name} {rule}", accepts)
    return torch.full((n,), number, dtype=torch.float64, device=device)


def affine_rows(n: int, in_size: tuple[int, int], out_size: tuple[int, int] | None = None, *, angle: Any = 0.0, scale: Any = 1.0, shear: Any = 0.0,
                translate: tuple[Any, Any] = (0.0, 0.0), flip: Any = False, device: str | torch.device | None = None) -> torch.Tensor:
    """(N, 6) float32 rows on ``device`` (default: that of the first tensor argument, else the CPU) for ``affine_warp``, from numbers or
    (N,) tensors: the content of an ``in_size = (H, W)`` tile is mirrored left-right where ``flip``, sheared by ``shear`` degrees along x,
    turned ANTICLOCKWISE by ``angle`` degrees (as ``torch.rot90(x, 1, (-2, -1))`` turns it at 90), magnified by ``scale`` (> 1 magnifies)
    and moved by ``translate = (tx, ty)`` pixels (right, down) -- about the tile centres ``((W - 1) / 2, (H - 1) / 2)`` of the source and
    ``((OW - 1) / 2, (OH - 1) / 2)`` of the output (``out_size``, default ``in_size``).  The formula, in float64 torch ops, rounded once to
    float32 -- no host copy, a call stays capturable:

        t = angle pi / 180, (cos, sin) = (cos t, sin t) -- for an angle that is a multiple of 90 taken from {0, 1, -1} by selection,
        so that quarter turns of square tiles are pixel permutations bit for bit;  k = tan(shear pi / 180);  m = -1 where flip else 1
        a = m (cos - k sin) / scale      b = m (-sin - k cos) / scale      d = sin / scale      e = cos / scale
        ux = (OW - 1) / 2 + tx           uy = (OH - 1) / 2 + ty
        c = (W - 1) / 2 - a ux - b uy    f = (H - 1) / 2 - d ux - e uy
    """
    n = fe.whole_number(n, "n must be a positive int", lo=1)
    h, w = _check_size(in_size, "in_size") or (None, None)
    if h is None:
        raise ValueError("in_size must be an (H, W) pair of positive ints, got None")
    oh, ow = _check_size(out_size, "out_size") or (h, w)
    if not isinstance(translate, (tuple, list)) or len(translate) != 2:
        raise ValueError(f"translate must be a (tx, ty) pair, got {translate!r}")
    given = [v for v in (angle, scale, shear, translate[0], translate[1], flip) if isinstance(v, torch.Tensor)]
    device = torch.device(device) if device is not None else (given[0].device if given else torch.device("cpu"))
    angle = _per_tile(angle, n, "angle", device)
    scale = _per_tile(scale, n, "scale", device, lambda v: math.isfinite(v) and v > 0.0, "must be finite and positive")
    shear = _per_tile(shear, n, "shear", device)
    tx, ty = _per_tile(translate[0], n, "translate x", device), _per_tile(translate[1], n, "translate y", device)
    if isinstance(flip, torch.Tensor):
        if tuple(flip.shape) not in ((), (n,)):
            raise ValueError(f"flip must be a bool or a tensor of shape () or (N,) = ({n},), got {tuple(flip.shape)}")
        flip = flip.to(device).expand(n) != 0
    else:
        flip = torch.full((n,), bool(flip), dtype=torch.bool, device=device)
    quarters = angle / 90.0
    turn = torch.round(quarters)
    quarter = quarters == turn
    k4 = torch.remainder(turn, 4.0)
    one, zero = torch.ones_like(angle), torch.zeros_like(angle)
    theta = angle * (math.pi / 180.0)
    cos = torch.where(quarter, torch.where(k4 == 0, one, torch.where(k4 == 2, -one, zero)), torch.cos(theta))
    sin = torch.where(quarter, torch.where(k4 == 1, one, torch.where(k4 == 3, -one, zero)), torch.sin(theta))
    k = torch.tan(shear * (math.pi / 180.0))
    m = torch.where(flip, -one, one)
    a, b, d, e = m * (cos - k * sin) / scale, m * (-sin - k * cos) / scale, sin / scale, cos / scale
    ux, uy = (ow - 1) / 2.0 + tx, (oh - 1) / 2.0 + ty
    c = (w - 1) / 2.0 - a * ux - b * uy
    f = (h - 1) / 2.0 - d * ux - e * uy
    return torch.stack([a, b, c, d, e, f], dim=1).to(torch.float32)


# ----------------------------------------------------------------------------------------------------------------- the module
def _range(name: str, value: Any, accepts=math.isfinite, rule: str = "finite") -> tuple[float, float]:
    if not isinstance(value, (tuple, list)) or len(value) != 2:
        raise ValueError(f"{name} must be a (lo, hi) pair, got {value!r}")
    lo, hi = (fe.real_number(v, f"{name} {end} must be a number", f"{name} {end} must be {rule}", accepts) for v, end in zip(value, ("lo", "hi")))
    if lo > hi:
        raise ValueError(f"{name} must be a (lo, hi) pair with lo <= hi, got {tuple(value)!r}")
    return lo, hi


class AffineAugment(nn.Module):
    """Random per-tile affine maps of CHW / NCHW tensors on an MI355X, one launch per batch.  Per tile: ``rotate=(lo, hi)`` degrees,
    anticlockwise, uniform -- or ``rotate="quarter"``: one of the four right angles, with ``flip=True`` the eight symmetries of Tellez et
    al.'s "basic" set, pixel permutations on square tiles --; ``scale=(lo, hi)`` uniform (> 1 magnifies); ``shear=(lo, hi)`` degrees;
    ``translate=(fx, fy)``: a shift uniform in ``[-fx OW, fx OW]`` x ``[-fy OH, fy OH]`` pixels, fractions of the output tile's sides;
    ``flip``: a left-right mirror (before the turn) with probability 1/2.  With probability ``1 - p`` a tile is left as it is (a NaN row:
    copied, or centre-cropped to ``size``; nothing is synchronised).  ``size=(OH, OW)``: the result's size, default the input's -- 224 out
    of 320 after a rotation shows no border.  ``interpolation``, ``border``, ``fill`` as ``affine_warp``; ``normalize_to_0_1`` (default
    True, as the sibling modules); ``generator`` drives ``sample_rows``; ``device=None`` follows the input tensor.  With a generator ON the
    device the rows are drawn and built there and a call enqueues no host copy."""

    def __init__(self, rotate: Any = (-180.0, 180.0), scale: tuple[float, float] = (1.0, 1.0), shear: tuple[float, float] = (0.0, 0.0), translate: tuple[float, float] = (0.0, 0.0),
                 flip: bool = True, *, p: float = 1.0, size: tuple[int, int] | None = None, interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0,
                 normalize_to_0_1: bool = True, generator: torch.Generator | None = None, device: str | torch.device | None = None):
        super().__init__()
        self.rotate = "quarter" if isinstance(rotate, str) and rotate == "quarter" else _range("rotate", rotate)
        self.scale = _range("scale", scale, lambda v: math.isfinite(v) and v > 0.0, "finite and positive")
        self.shear = _range("shear", shear, lambda v: math.isfinite(v) and -90.0 < v < 90.0, "in (-90, 90) degrees")
        if not isinstance(translate, (tuple, list)) or len(translate) != 2:
            raise ValueError(f"translate must be an (fx, fy) pair of fractions, got {translate!r}")
        self.translate = tuple(fe.real_number(v, f"translate {axis} must be a number", f"translate {axis} must be a finite fraction >= 0", lambda t: math.isfinite(t) and t >= 0.0)
                               for v, axis in zip(translate, ("fx", "fy")))
        self.flip = bool(flip)
        self.p = fe.real_number(p, "p must be a number in [0, 1]", "p must lie in [0, 1]", lambda v: 0.0 <= v <= 1.0, show=float)
        self.size = _check_size(size)
        self.interpolation = _check_choice("interpolation", interpolation, INTERPOLATIONS)
        self.border = _check_choice("border", border, BORDERS)
        self.fill = _check_fill(fill)
        self.device = fe.cuda_only(device, "AffineAugment")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator

    def sample_rows(self, n: int, in_size: tuple[int, int], device: str | torch.device | None = None) -> torch.Tensor:
        """(n, 6) float32 rows on ``device`` for tiles of ``in_size = (H, W)``, drawn with the module's generator (on the generator's
        device, then moved) and built by ``affine_rows``.  SIX draws of ``rand(n)``, always and in this order: the angle (``lo + (hi - lo)
        u``, or ``90 floor(4 u)`` for ``"quarter"``), the scale (``lo + (hi - lo) u``), the shear (likewise), the shift along x (``(2 u -
        1) fx OW``) and along y (``(2 u - 1) fy OH``), the flip (``u < 0.5``, used where ``flip=True``).  ``p < 1``: one more draw,
        ``rand(n) < p``; a tile that is not chosen gets a row of NaNs."""
        device = fe.draw_device(device, self.device)
        h, w = _check_size(in_size, "in_size")
        oh, ow = self.size or (h, w)
        u = [fe.draw(self.generator, (n,), device).to(device).to(torch.float64) for _ in range(6)]
        angle = 90.0 * torch.floor(4.0 * u[0]) if self.rotate == "quarter" else self.rotate[0] + (self.rotate[1] - self.rotate[0]) * u[0]
        scale = self.scale[0] + (self.scale[1] - self.scale[0]) * u[1]
        shear = self.shear[0] + (self.shear[1] - self.shear[0]) * u[2]
        tx, ty = (2.0 * u[3] - 1.0) * (self.translate[0] * ow), (2.0 * u[4] - 1.0) * (self.translate[1] * oh)
        flip = (u[5] < 0.5) if self.flip else torch.zeros((n,), dtype=torch.bool, device=device)
        rows = affine_rows(n, (h, w), (oh, ow), angle=angle, scale=scale, shear=shear, translate=(tx, ty), flip=flip, device=device)
        if self.p < 1.0:
            rows = torch.where(fe.chosen(self.generator, n, self.p, device), rows, torch.full_like(rows, float("nan")))
        return rows

    def forward(self, img: torch.Tensor, rows: torch.Tensor | None = None, mask: Any = None) -> Any:
        """``rows``: explicit (6,), (1, 6) or (N, 6) rows instead of a draw.  ``mask``: a uint8 / bool tensor (N, H, W) or (N, 1, H, W)
        that is warped WITH the tiles (nearest, the module's border, 0 outside): the result is ``(tiles, warped mask)`` -- two launches,
        the same rows."""
        if rows is None:
            batch, _, (n, h, w) = fe.image_batch(img, False, "AffineAugment")
            rows = self.sample_rows(n, (h, w), fe.run_device(self.device, batch.device, "AffineAugment"))
        return _warp(img, rows, "AffineAugment", size=self.size, interpolation=self.interpolation, border=self.border, fill=self.fill, channels_last=False,
                     normalize_to_0_1=self.normalize_to_0_1, out_dtype=None, device=self.device, mask=mask)

    def extra_repr(self) -> str:
        return (f"rotate={self.rotate!r}, scale={self.scale}, shear={self.shear}, translate={self.translate}, flip={self.flip}, p={self.p}, size={self.size}, "
                f"interpolation={self.interpolation!r}, border={self.border!r}, fill={self.fill}, normalize_to_0_1={self.normalize_to_0_1}")
