"""Three-stain colour deconvolution with a GIVEN basis (an extension: the reference has none).

Ruifrok & Johnston's colour deconvolution as HistomicsTK's ``color_deconvolution``, scikit-image's ``rgb2hed`` / ``hed2rgb`` and the
fixed-matrix augmentors of tiatoolbox / torchstain offer it: the optical density of a pixel is split into THREE stain concentrations
by the inverse of a fixed (3, 3) basis -- no estimate, so it serves IHC slides (haematoxylin + DAB) that Macenko's H&E estimate does
not, and it is lossless: the concentrations can be edited and the tile rebuilt.  ``ColorDeconvolution`` separates, applies
(``C' = alpha * C + beta``, optionally rebuilt with another basis) and combines; ``HEDAugment`` is the "HED-light" jitter of Tellez et
al. as an ``nn.Module``; ``ColorDeconvolution.quantify`` measures a slide -- integer histograms of the three concentrations
(``StainHistograms``: positive-pixel fraction, H-score, mean, percentiles) in one streaming launch that writes no map.  The conventions are the Macenko calls' (``OD = -ln((255 x + 1) / 240)``, ``level = clamp(240 exp(-OD'))``), so
an estimated H&E basis, complemented (``StainEstimate.complement()``), feeds the same path with the residual as a channel of its own.
One kernel launch per call (include/stainx_hip.h: sx_deconv_*).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, NamedTuple

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks

# (H, E or DAB, third) as Ruifrok & Johnston tabulate them; a missing third vector is the complement of the first two
_NAMED = {
    "hed": ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78)),
    "he": ((0.644211, 0.716556, 0.266844), (0.092789, 0.954111, 0.283111), None),
    "hdab": ((0.650, 0.704, 0.286), (0.268, 0.570, 0.776), None),
}
BASIS_NAMES = tuple(_NAMED)


def complement_basis(he: torch.Tensor) -> torch.Tensor:
    """``(..., 3, 2)`` stain vectors (columns, as ``HE_source``) -> ``(..., 3, 3)``: the two columns as they are, the third their
    normalised cross product (HistomicsTK's ``complement_stain_matrix``) -- orthogonal to both, unit length, right-handed.  So the
    first two rows of the inverse are the pseudo-inverse of ``he``, and the third concentration is the residual the rank-2 path drops.
    Plain tensor arithmetic on the tensor's device (no synchronisation)."""
    if not isinstance(he, torch.Tensor) or he.dim() < 2 or tuple(he.shape[-2:]) != (3, 2):
        raise ValueError(f"complement_basis expects (..., 3, 2) stain vectors, got {tuple(getattr(he, 'shape', ()))}")
    he = he.to(torch.float32)
    third = torch.linalg.cross(he[..., 0], he[..., 1], dim=-1)
    third = third / torch.linalg.vector_norm(third, dim=-1, keepdim=True)
    return torch.cat([he, third.unsqueeze(-1)], dim=-1)


def stain_basis(name_or_matrix: Any) -> torch.Tensor:
    """A (3, 3) float32 basis, ``[channel][stain]``, with unit-length columns: one of the built-in names -- ``"hed"`` (Ruifrok &
    Johnston's haematoxylin, eosin, DAB), ``"he"`` and ``"hdab"`` (two stains and their complement) -- or a given matrix.  A CPU
    matrix is checked here (shape (3, 3) or (N, 3, 3), finite, non-zero determinant) and its columns normalised; a device tensor is
    taken as it is, with no synchronisation (a singular basis is not detected on the device: the result is then undefined)."""
    if isinstance(name_or_matrix, str):
        if name_or_matrix not in _NAMED:
            raise ValueError(f"unknown stain basis {name_or_matrix!r}; built in: {list(BASIS_NAMES)} (or pass a (3, 3) matrix)")
        first, second, third = _NAMED[name_or_matrix]
        cols = torch.tensor([first, second], dtype=torch.float64).T      # (3, 2)
        cols = cols / torch.linalg.vector_norm(cols, dim=0, keepdim=True)
        if third is None:
            c = torch.linalg.cross(cols[:, 0], cols[:, 1])
        else:
            c = torch.tensor(third, dtype=torch.float64)
        c = c / torch.linalg.vector_norm(c)
        return torch.cat([cols, c.unsqueeze(1)], dim=1).to(torch.float32)
    m = name_or_matrix
    if not isinstance(m, torch.Tensor):
        try:
            m = torch.as_tensor(m, dtype=torch.float32)
        except Exception:
            raise ValueError(f"a stain basis is a name ({list(BASIS_NAMES)}) or a (3, 3) matrix, got {type(name_or_matrix).__name__}") from None
    if not (tuple(m.shape) == (3, 3) or (m.dim() == 3 and tuple(m.shape[1:]) == (3, 3) and m.shape[0] >= 1)):
        raise ValueError(f"a stain basis must have shape (3, 3) or (N, 3, 3), [channel][stain], got {tuple(m.shape)}")
    if not m.dtype.is_floating_point:
        m = m.to(torch.float32)
    if m.device.type != "cpu":
        return m.to(torch.float32)
    m64 = m.to(torch.float64)
    if not bool(torch.isfinite(m64).all()):
        raise ValueError("a stain basis must be finite")
    if bool((torch.linalg.det(m64).abs() < 1e-12).any()):
        raise ValueError("a stain basis must be invertible (its determinant is zero: two stain vectors are parallel, or one is zero)")
    return (m64 / torch.linalg.vector_norm(m64, dim=-2, keepdim=True)).to(torch.float32)


@dataclass
class DeconvSeparation:
    """What ``ColorDeconvolution.separate`` returns; a field that was not asked for is None.
    ``images``: (3, N, 3, H, W) -- (3, N, H, W, 3) with ``channel_axis=-1`` --, image i the tile rebuilt from stain i alone.
    ``concentrations``: (N, 3, H, W) float32 ((N, H, W, 3)).  ``basis``: the (3, 3) or (N, 3, 3) basis used."""

    images: torch.Tensor | None
    concentrations: torch.Tensor | None
    basis: torch.Tensor


def _check_binning(bin_log2: Any, zero_bin: Any) -> tuple[int, int]:
    return (fe.whole_number(bin_log2, "bin_log2 must be an integer in [0, 8] (bins of width 2^-bin_log2)", 0, 8),
            fe.whole_number(zero_bin, "zero_bin must be an integer in [0, 255] (the bin whose lower edge is concentration 0)", 0, 255))


class StainHistograms(NamedTuple):
    """What ``ColorDeconvolution.quantify`` returns: integer histograms of the three stain concentrations of a batch, estimated in one
    streaming launch -- no concentration map is written.  ``counts``: (S, 3, 256) int64, bin b of stain s of set S; ``sums``: (S, 3)
    int64, the sum of the concentrations in fixed point (units of 2^-16); ``pixels``: (S,) int64, the pixels counted (finite
    concentrations, and inside the mask if there is one).  S = N for a set per tile, 1 for one set pooled over the batch.  Bin b covers
    ``[(b - zero_bin) 2^-bin_log2, (b + 1 - zero_bin) 2^-bin_log2)``; bins 0 and 255 also take everything below / above that range.

    Everything is an integer, so results are the same run to run and sets of different batches, slides or ranks ADD UP EXACTLY
    (:meth:`pool`, or ``all_reduce`` (SUM) on the three tensors).  The derived figures are plain torch ops where the tensors live (no
    synchronisation).  The thresholds of :meth:`positive_fraction` and :meth:`h_score` must be bin edges: the figures are then exact --
    the same numbers a threshold on the concentration map gives."""

    counts: torch.Tensor
    sums: torch.Tensor
    pixels: torch.Tensor
    bin_log2: int = 5
    zero_bin: int = 64

    @staticmethod
    def pool(*items: "StainHistograms") -> "StainHistograms":
        """One set, (1, 3, 256), (1, 3) and (1,): the sum of every set of every argument (exact).  ValueError on differing binning."""
        if not items:
            raise ValueError("pool needs at least one StainHistograms")
        first = items[0]
        counts = sums = pixels = None
        for item in items:
            if not isinstance(item, StainHistograms):
                raise ValueError(f"pool takes StainHistograms, got {type(item).__name__}")
            if (item.bin_log2, item.zero_bin) != (first.bin_log2, first.zero_bin):
                raise ValueError(f"pool: the sets are binned differently (bin_log2, zero_bin) = {(first.bin_log2, first.zero_bin)} and {(item.bin_log2, item.zero_bin)}; "
                                 "counts of different bins do not add up")
            c, s, p = item.counts.sum(dim=0, keepdim=True), item.sums.sum(dim=0, keepdim=True), item.pixels.sum(dim=0, keepdim=True)
            counts, sums, pixels = (c, s, p) if counts is None else (counts + c, sums + s, pixels + p)
        return StainHistograms(counts, sums, pixels, first.bin_log2, first.zero_bin)

    def edges(self) -> torch.Tensor:
        """(257,) float64: the bin edges, ``(b - zero_bin) 2^-bin_log2`` for b = 0 .. 256."""
        return (torch.arange(257, dtype=torch.float64, device=self.counts.device) - self.zero_bin) / float(1 << self.bin_log2)

    def mean(self) -> torch.Tensor:
        """(S, 3) float64: the mean concentration of each stain over the counted pixels, ``sums / 2^16 / pixels``; 0 where nothing was counted."""
        p = self.pixels.to(torch.float64).unsqueeze(-1)
        return torch.where(p > 0, self.sums.to(torch.float64) / 65536.0 / p.clamp(min=1.0), torch.zeros_like(p))

    def _edge(self, threshold: Any, name: str = "threshold") -> int:
        """The index e (1 .. 255) of the bin edge ``threshold`` is: ``C >= threshold`` is then ``bin >= e``, exactly."""
        try:
            t = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {threshold!r}") from None
        scale = float(1 << self.bin_log2)
        pos = t * scale      # (exact for every float that is an edge)
        if not math.isfinite(t) or pos != math.floor(pos) or not 1 <= int(pos) + self.zero_bin <= 255:
            lo, hi = (1 - self.zero_bin) / scale, (255 - self.zero_bin) / scale
            if math.isfinite(t):
                below, above = min(max(math.floor(pos) / scale, lo), hi), min(max(math.ceil(pos) / scale, lo), hi)
                near = f"the nearest edges are {below!r} and {above!r}" if below != above else f"the nearest edge is {below!r}"
            else:
                near = "it is not finite"
            raise ValueError(f"{name} = {threshold!r} is not a bin edge inside the range: edges are multiples of {1.0 / scale!r} from {lo!r} to {hi!r}; {near} "
                             "(a threshold between two edges cannot be answered exactly from a histogram)")
        return int(pos) + self.zero_bin

    @staticmethod
    def _stain(stain: Any) -> int:
        return fe.whole_number(stain, "stain must be 0, 1 or 2 (a column of the basis)", 0, 2)

    def _at_least(self, stain: int, edge: int) -> torch.Tensor:
        return self.counts[:, stain, edge:].sum(dim=-1)

    def _share(self, numerator: torch.Tensor, factor: float) -> torch.Tensor:
        p = self.pixels.to(torch.float64)
        return torch.where(p > 0, factor * numerator.to(torch.float64) / p.clamp(min=1.0), torch.zeros_like(p))

    def positive_fraction(self, stain: int, threshold: float) -> torch.Tensor:
        """(S,) float64: the share of the counted pixels with ``C_stain >= threshold`` (the positive-pixel fraction; DAB area fraction
        with ``stain=1`` of ``"hdab"``); 0 where nothing was counted.  ``threshold`` must be a bin edge inside the range."""
        return self._share(self._at_least(self._stain(stain), self._edge(threshold)), 1.0)

    def h_score(self, stain: int, thresholds: tuple[float, float, float]) -> torch.Tensor:
        """(S,) float64 in [0, 300]: the pixel-wise H-score ``100 (weak + 2 moderate + 3 strong) / pixels`` with weak = ``[t1, t2)``,
        moderate = ``[t2, t3)``, strong = ``>= t3``; 0 where nothing was counted.  ``thresholds``: three ascending bin edges."""
        stain = self._stain(stain)
        if not isinstance(thresholds, (tuple, list)) or len(thresholds) != 3:
            raise ValueError(f"thresholds must be three ascending bin edges (t1, t2, t3), got {thresholds!r}")
        e = [self._edge(t, f"thresholds[{i}]") for i, t in enumerate(thresholds)]
        if not e[0] <= e[1] <= e[2]:
            raise ValueError(f"thresholds must be ascending, got {tuple(thresholds)!r}")
        # (weak + 2 moderate + 3 strong = the pixels at or above t1, plus those at or above t2, plus those at or above t3)
        return self._share(self._at_least(stain, e[0]) + self._at_least(stain, e[1]) + self._at_least(stain, e[2]), 100.0)

    def quantile(self, stain: int, q: float) -> torch.Tensor:
        """(S,) float64: the lower edge of the bin that holds the nearest-rank element of ``C_stain`` -- rank ``max(1, ceil(q pixels))``
        in ascending order --; NaN where nothing was counted.  Within one bin width of the exact quantile for values inside the range."""
        stain = self._stain(stain)
        try:
            q = float(q)
        except (TypeError, ValueError):
            raise ValueError(f"q must be a number in [0, 1], got {q!r}") from None
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q must lie in [0, 1], got {q!r}")
        rank = torch.ceil(q * self.pixels.to(torch.float64)).to(torch.int64).clamp(min=1)
        cumulative = self.counts[:, stain].cumsum(dim=-1)
        index = torch.searchsorted(cumulative, rank.unsqueeze(-1)).squeeze(-1).clamp(max=255)      # the first bin whose cumulative count reaches the rank
        value = (index.to(torch.float64) - self.zero_bin) / float(1 << self.bin_log2)
        return torch.where(self.pixels > 0, value, torch.full_like(value, float("nan")))


class ConcentrationStatistics(NamedTuple):
    """What ``ColorDeconvolution.estimate`` returns: exact integer moments of the three stain concentrations of a batch, taken in one
    streaming launch -- no concentration map is written.  ``sums``: (S, 3) int64, the sum of the concentrations in fixed point (units of
    2^-16, ``quantify``'s sums); ``squares``: (S, 3) int64, the sum of their squares (units of 2^-24, each pixel's term floored; a
    concentration beyond +-64 enters as 64); ``pixels``: (S,) int64, the pixels counted (finite concentrations, and inside the mask if
    there is one).  S = N for a set per tile, 1 for one set pooled over the batch.

    Integers throughout: the same run to run, and sets of different tiles, batches, slides or ranks ADD UP EXACTLY (:meth:`pool`, or
    ``all_reduce`` (SUM) on the three tensors).  :meth:`mean` and :meth:`std` are float64 torch ops where the tensors live (no
    synchronisation)."""

    sums: torch.Tensor
    squares: torch.Tensor
    pixels: torch.Tensor

    @staticmethod
    def pool(*items: "ConcentrationStatistics") -> "ConcentrationStatistics":
        """One set, (1, 3), (1, 3) and (1,): the sum of every set of every argument (exact)."""
        if not items:
            raise ValueError("pool needs at least one ConcentrationStatistics")
        sums = squares = pixels = None
        for item in items:
            if not isinstance(item, ConcentrationStatistics):
                raise ValueError(f"pool takes ConcentrationStatistics, got {type(item).__name__}")
            s, q, p = item.sums.sum(dim=0, keepdim=True), item.squares.sum(dim=0, keepdim=True), item.pixels.sum(dim=0, keepdim=True)
            sums, squares, pixels = (s, q, p) if sums is None else (sums + s, squares + q, pixels + p)
        return ConcentrationStatistics(sums, squares, pixels)

    def _mean_std(self) -> tuple[torch.Tensor, torch.Tensor]:
        """``(mean(), std())`` in one go (the two share half of their operations)."""
        p = self.pixels.to(torch.float64).unsqueeze(-1)
        some = p.clamp(min=1.0)
        s = self.sums.to(torch.float64) * (1.0 / 65536.0)      # (a power of two: the product is the quotient)
        q = self.squares.to(torch.float64) * (1.0 / 16777216.0)
        mean = s / some
        var = (q - s * mean) / (some - 1.0).clamp(min=1.0)
        sd = torch.sqrt(var.clamp(min=0.0))
        none = p < 2.0
        return mean.masked_fill(none, float("nan")), sd.masked_fill(none, float("nan"))

    def mean(self) -> torch.Tensor:
        """(S, 3) float64: the mean concentration of each stain over the counted pixels, ``sums / 2^16 / pixels``; NaN where fewer than
        two pixels were counted (a set without statistics, as ``Reinhard.estimate``'s NaN rows)."""
        return self._mean_std()[0]

    def std(self) -> torch.Tensor:
        """(S, 3) float64: the unbiased standard deviation, ``sqrt((squares / 2^24 - (sums / 2^16) mean) / (pixels - 1))`` (a negative
        difference -- the floor of the squares on a constant tile -- counts as 0); NaN where fewer than two pixels were counted."""
        return self._mean_std()[1]


def _statistics_rows(value: Any, n: int, what: str) -> tuple[torch.Tensor, torch.Tensor]:
    """``(mean, std)`` of a ``ConcentrationStatistics`` or a given pair, each (3,), (1, 3) or (N, 3): checked by shape only (no GPU work)."""
    if isinstance(value, ConcentrationStatistics):
        rows = tuple(value.pixels.shape)
        if len(rows) != 1 or rows[0] not in (1, n) or tuple(value.sums.shape) != (rows[0], 3) or tuple(value.squares.shape) != (rows[0], 3):
            raise ValueError(f"{what} holds {rows} sets for a batch of {n} tiles (one set, or one per tile)")
        return value._mean_std()
    return fe.mean_std_rows(value, n, what, "ConcentrationStatistics")


def check_gain_range(gain_range: Any) -> tuple[float, float]:
    try:
        lo, hi = (float(g) for g in gain_range)
    except (TypeError, ValueError):
        raise ValueError(f"gain_range must be a pair (low, high) with 0 < low <= high, got {gain_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"gain_range must be a pair (low, high) with 0 < low <= high, got {gain_range!r}")
    return lo, hi


def match_factors(source_mean: torch.Tensor, source_std: torch.Tensor, target_mean: torch.Tensor, target_std: torch.Tensor, n: int,
                  gain_range: tuple[float, float]) -> tuple[torch.Tensor, torch.Tensor]:
    """``(alpha, beta)``, (n, 3) float32 each, where the statistics live: ``alpha = clamp(target_std / source_std, gain_range)``,
    ``beta = target_mean - alpha * source_mean``, in float32.  A tile whose source row holds a NaN or a zero standard deviation -- or
    whose target row holds a NaN -- gets ``alpha = 1, beta = 0`` for all three stains.  Plain torch ops, no synchronisation."""
    sm, ss, tm, ts = (t.to(torch.float32).reshape(-1, 3).expand(n, 3) for t in (source_mean, source_std, target_mean, target_std))
    alpha = torch.clamp(ts / ss, gain_range[0], gain_range[1])
    beta = tm - alpha * sm
    leave = (torch.isnan(torch.cat([sm, ss, tm, ts], dim=1)).any(dim=1, keepdim=True)) | (ss == 0).any(dim=1, keepdim=True)
    return alpha.masked_fill(leave, 1.0), beta.masked_fill(leave, 0.0)


def _check_factor(name: str, factor: Any, n: int) -> None:
    if factor is not None and (not isinstance(factor, torch.Tensor) or tuple(factor.shape) != (n, 3)):
        raise ValueError(f"{name} must be a tensor of shape (N, 3) = ({n}, 3), got {tuple(getattr(factor, 'shape', ()))}")


class ColorDeconvolution:
    """Separate, apply and combine with a given three-stain basis on an MI355X.

    ``basis`` / ``target``: what ``stain_basis`` takes -- a name, a (3, 3) matrix, or per-tile (N, 3, 3) bases (a
    ``StainEstimate.complement()``); with ``target`` ``apply`` rebuilds the tile with that basis (stain transfer between two fixed
    bases).  ``channel_axis=-1``: NHWC tiles in and out (unmasked calls only).  ``normalize_to_0_1``: uint8 tiles come out as float32
    in [0, 1], float tiles are divided by 255.  ``mask="luminosity"`` (or ``apply(..., mask=tensor)``): only tissue pixels are
    changed, the others are copied by the masked transforms' background rule.  ``device=None`` follows the input tensor.  All argument
    errors are raised before any GPU work."""

    def __init__(self, basis: Any = "hed", *, target: Any = None, device: str | torch.device | None = None, channel_axis: int = 1, normalize_to_0_1: bool = False,
                 mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        self.basis = stain_basis(basis)
        self.target = None if target is None else stain_basis(target)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.channels_last = fe.channels_last(channel_axis)
        if self.channels_last and self.mask is not None:
            raise ValueError("a masked deconvolution takes planar (NCHW) tiles only: mask= with channel_axis=-1 is not supported")
        self.channel_axis = channel_axis
        self.device = fe.cuda_only(device, "ColorDeconvolution")
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self._engines: dict[torch.device, Any] = {}
        self._device_bases: dict[torch.device, tuple[torch.Tensor, torch.Tensor | None]] = {}

    def _upload(self, device: torch.device) -> tuple[torch.Tensor, torch.Tensor | None]:
        return tuple(None if b is None else b.to(device=device, dtype=torch.float32).contiguous() for b in (self.basis, self.target))

    def _bases_on(self, device: torch.device) -> tuple[torch.Tensor, torch.Tensor | None]:
        """The basis and the target as float32 tensors on ``device``, uploaded ONCE per device (a host basis copied in front of every
        call would put a pageable copy before the one launch, and keep a call from being captured)."""
        return fe.held(self._device_bases, device, self._upload)

    def _engine(self, device: torch.device):
        return fe.held(self._engines, device, fe.engine, "DeconvHIP")

    def _batch(self, x: Any, what: str) -> tuple[torch.Tensor, bool, tuple[int, int, int]]:
        return fe.image_batch(x, self.channels_last, what)

    def _masking(self, mask: Any, single: bool, dims: tuple[int, int, int], batch: torch.Tensor) -> tuple[torch.Tensor | None, float] | None:
        """The engine's ``masking=`` for a call -- ``(explicit mask or None, threshold)``, None when unmasked -- after the mask's checks."""
        masked, explicit = fe.call_mask(self.mask, mask, single, dims, self.device or batch.device, self.channels_last, "deconvolution")
        return (explicit, self.luminosity_threshold) if masked else None

    def _rows_ok(self, n: int) -> None:
        for name, b in (("basis", self.basis), ("target", self.target)):
            if b is not None and b.dim() == 3 and b.shape[0] not in (1, n):
                raise ValueError(f"{name} holds {b.shape[0]} bases for a batch of {n} tiles (one basis, or one per tile)")

    def separate(self, x: torch.Tensor, stains: bool = True, concentrations: bool = False) -> DeconvSeparation:
        batch, single, _ = self._batch(x, "separate")
        if not stains and not concentrations:
            raise ValueError("separate: ask for the stain images (stains=True), the concentrations, or both")
        self._rows_ok(batch.shape[0])
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        imgs, conc = self._engine(device).separate(batch, self._bases_on(device)[0], stains=stains, concentrations=concentrations, normalize_to_0_1=self.normalize_to_0_1,
                                                   channels_last=self.channels_last)
        if single:
            imgs = None if imgs is None else imgs.squeeze(1)
            conc = None if conc is None else conc.squeeze(0)
        return DeconvSeparation(imgs, conc, self.basis)

    def apply(self, x: torch.Tensor, alpha: torch.Tensor | None = None, beta: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        """``alpha`` / ``beta``: (N, 3) per-tile factors of the three concentrations, both or neither.  ``mask``: an explicit uint8 /
        bool tensor (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call."""
        batch, single, (n, h, w) = self._batch(x, "apply")
        if (alpha is None) != (beta is None):
            raise ValueError("alpha and beta go together: both or neither")
        _check_factor("alpha", alpha, n)
        _check_factor("beta", beta, n)
        self._rows_ok(n)
        masking = self._masking(mask, single, (n, h, w), batch)
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        out = self._engine(device).apply(batch, *self._bases_on(device), alpha=alpha, beta=beta, normalize_to_0_1=self.normalize_to_0_1, channels_last=self.channels_last,
                                         masking=masking)
        return out.squeeze(0) if single else out

    def quantify(self, x: torch.Tensor, *, pooled: bool = False, bin_log2: int = 5, zero_bin: int = 64, mask: Any = None) -> StainHistograms:
        """Measure instead of map: the 256-bin integer histograms of the three concentrations ``separate(x, concentrations=True)`` would
        write (bit for bit those values), their fixed-point sums and the counted pixels -- a set per tile, or one set ``pooled`` over the
        batch -- in ONE streaming launch that reads a pixel once and writes no map.  Bins are ``2^-bin_log2`` wide and bin ``zero_bin``
        starts at concentration 0 (defaults: 1/32 over [-2, 6)).  ``mask``: as in ``apply`` -- only masked-in pixels count.  Pixels with a
        non-finite concentration (NaN / Inf input, ``255 x + 1 <= 0``) are not counted.  See ``StainHistograms`` for the figures."""
        batch, single, (n, h, w) = self._batch(x, "quantify")
        bin_log2, zero_bin = _check_binning(bin_log2, zero_bin)
        self._rows_ok(n)
        masking = self._masking(mask, single, (n, h, w), batch)
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        counts, sums, pixels = self._engine(device).quantify(batch, self._bases_on(device)[0], bin_log2=bin_log2, zero_bin=zero_bin, per_tile=not pooled,
                                                             channels_last=self.channels_last, masking=masking)
        return StainHistograms(counts, sums, pixels, bin_log2, zero_bin)

    def estimate(self, x: torch.Tensor, *, pooled: bool = False, mask: Any = None) -> ConcentrationStatistics:
        """The statistics pass of the stain space: exact integer sums and sums of squares of the three concentrations
        ``separate(x, concentrations=True)`` would write (bit for bit those values) and the counted pixels -- a set per tile, or one set
        ``pooled`` over the batch -- in ONE streaming launch that reads a pixel once and writes no map (include/stainx_hip.h:
        sx_deconv_moments).  ``mask``: as in ``apply`` -- only masked-in pixels count.  See ``ConcentrationStatistics``."""
        batch, single, (n, h, w) = self._batch(x, "estimate")
        self._rows_ok(n)
        masking = self._masking(mask, single, (n, h, w), batch)
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        return ConcentrationStatistics(*self._engine(device).moments(batch, self._bases_on(device)[0], per_tile=not pooled, channels_last=self.channels_last,
                                                                     masking=masking))

    def match(self, x: torch.Tensor, source: Any, target: Any, *, mask: Any = None, gain_range: tuple[float, float] = (0.1, 2.5)) -> torch.Tensor:
        """Mean / standard deviation matching of the concentrations ("Reinhard in stain space"): ``C' = alpha * C + beta`` with
        ``alpha = clamp(target_std / source_std, gain_range)`` and ``beta = target_mean - alpha * source_mean`` per tile and stain, then
        ``apply``: one launch.  ``source`` / ``target``: a ``ConcentrationStatistics`` (``estimate``'s) or a ``(mean, std)`` pair of
        (3,), (1, 3) or (N, 3) tensors.  The factors are computed in float32 on the device: no synchronisation, the call is capturable.  A
        tile whose source row holds a NaN or a zero standard deviation (or whose target row holds a NaN) is mapped with ``alpha = 1,
        beta = 0``."""
        batch, single, (n, h, w) = self._batch(x, "match")
        gain_range = check_gain_range(gain_range)
        self._rows_ok(n)
        self._masking(mask, single, (n, h, w), batch)
        sm, ss = _statistics_rows(source, n, "source")
        tm, ts = _statistics_rows(target, n, "target")
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        alpha, beta = match_factors(sm.to(device), ss.to(device), tm.to(device), ts.to(device), n, gain_range)
        return self.apply(x, alpha, beta, mask=mask)

    def combine(self, concentrations: torch.Tensor, out_dtype: torch.dtype = torch.uint8) -> torch.Tensor:
        """``separate``'s inverse: (N, 3, H, W) float32 concentrations -> tiles of ``out_dtype``, rebuilt with ``basis``."""
        batch, single, _ = self._batch(concentrations, "combine")
        if batch.dtype != torch.float32:
            raise ValueError(f"concentrations must be float32, got {batch.dtype}")
        if out_dtype not in (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError(f"out_dtype must be uint8, float16, bfloat16, float32 or float64, got {out_dtype}")
        if self.normalize_to_0_1 and out_dtype == torch.uint8:
            raise ValueError("normalize_to_0_1 needs a float out_dtype in combine (uint8 output stays on 0-255)")
        self._rows_ok(batch.shape[0])
        device = fe.run_device(self.device, batch.device, "ColorDeconvolution")
        out = self._engine(device).combine(batch, self._bases_on(device)[0], out_dtype=out_dtype, normalize_to_0_1=self.normalize_to_0_1, channels_last=self.channels_last)
        return out.squeeze(0) if single else out

    def __repr__(self) -> str:
        return (f"ColorDeconvolution(basis={tuple(self.basis.shape)}, target={None if self.target is None else tuple(self.target.shape)}, channel_axis={self.channel_axis}, "
                f"normalize_to_0_1={self.normalize_to_0_1}, mask={self.mask!r})")


def _sigma3(name: str, sigma: Any, upper: float | None) -> tuple[float, float, float]:
    try:
        values = tuple(float(s) for s in sigma) if isinstance(sigma, (tuple, list)) else (float(sigma),) * 3
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a per-stain triple, got {sigma!r}") from None
    if len(values) != 3:
        raise ValueError(f"{name} must be a number or a per-stain triple, got {len(values)} values")
    for v in values:
        if not math.isfinite(v) or v < 0.0 or (upper is not None and v >= upper):
            bound = f"lie in [0, {upper})" if upper is not None else "be >= 0"
            raise ValueError(f"{name} must be finite and {bound}, got {sigma!r}")
    return values


class HEDAugment(nn.Module):
    """Random per-tile jitter of the three concentrations of a FIXED basis ("HED-light", Tellez et al.): ``C' = alpha * C + beta`` with
    ``alpha ~ U[1 - sigma1, 1 + sigma1]``, ``beta ~ U[-sigma2, sigma2]`` per tile and stain.  No estimate: one streaming launch per
    batch, on any stain (IHC included) and on tiles Macenko cannot estimate.  ``sigma1`` / ``sigma2``: a number or a per-stain triple.
    CHW / NCHW tensors; ``normalize_to_0_1`` (default True, as ``MacenkoAugment``); ``generator`` drives ``sample_factors``;
    ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): only tissue pixels are jittered.  The basis and the sigmas are uploaded once per
    device; with a generator ON the device the factors are drawn there and a call enqueues no host copy at all (the default CPU generator
    draws on the host and copies 6 N floats per call, as ``MacenkoAugment`` does).  The factors never leave the device."""

    def __init__(self, sigma1: Any = 0.05, sigma2: Any = 0.05, *, basis: Any = "hed", device: str | torch.device | None = None, normalize_to_0_1: bool = True,
                 generator: torch.Generator | None = None, mask: str | None = None, luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD):
        super().__init__()
        self.sigma1 = _sigma3("sigma1", sigma1, 1.0)
        self.sigma2 = _sigma3("sigma2", sigma2, None)
        self.generator = generator
        self.deconv = ColorDeconvolution(basis, device=device, normalize_to_0_1=normalize_to_0_1, mask=mask, luminosity_threshold=luminosity_threshold)
        self.device = self.deconv.device
        self._sigmas: dict[torch.device, tuple[torch.Tensor, torch.Tensor]] = {}      # (the per-stain sigmas on a device: uploaded once)

    def sample_factors(self, n: int, device: str | torch.device | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(alpha, beta)``, each (n, 3) float32 on ``device`` (exactly 1 and 0 for sigma = 0), drawn with the module's generator (on
        the generator's device, then moved), as ``MacenkoAugment.sample_factors`` draws them."""
        device = fe.draw_device(device, self.device)
        u = fe.draw(self.generator, (2, n, 3), device).to(device)
        s1, s2 = fe.held(self._sigmas, device, lambda device: tuple(torch.tensor(s, dtype=torch.float32, device=device) for s in (self.sigma1, self.sigma2)))
        return 1.0 + s1 * (2.0 * u[0] - 1.0), s2 * (2.0 * u[1] - 1.0)

    def forward(self, img: torch.Tensor, alpha: torch.Tensor | None = None, beta: torch.Tensor | None = None, mask: Any = None) -> torch.Tensor:
        batch, _, (n, _, _) = self.deconv._batch(img, "HEDAugment")
        _check_factor("alpha", alpha, n)
        _check_factor("beta", beta, n)
        if alpha is None or beta is None:
            device = fe.run_device(self.device, batch.device, "HEDAugment")
            drawn = self.sample_factors(n, device)
            alpha = drawn[0] if alpha is None else alpha
            beta = drawn[1] if beta is None else beta
        return self.deconv.apply(img, alpha, beta, mask=mask)      # (a single tile: apply adds and drops the batch axis, of the tile and of its mask)

    def extra_repr(self) -> str:
        return f"sigma1={self.sigma1}, sigma2={self.sigma2}, normalize_to_0_1={self.deconv.normalize_to_0_1}, mask={self.deconv.mask!r}"
