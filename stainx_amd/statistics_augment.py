"""Statistics-space stain augmentation (an extension: the reference has none).

RandStainNA (Shen et al., MICCAI 2022): every tile is moved, Reinhard-style, from its OWN channel statistics to statistics drawn per
tile from a distribution fitted to the cohort -- in LAB, or in HED on the concentrations of a fixed basis.  ``StatisticsDistribution``
holds the cohort's distribution (centres and spreads of the per-tile means and standard deviations), ``StatisticsAugment`` is the
``nn.Module`` beside ``MacenkoAugment`` and ``HEDAugment``.  The parts are the library's: ``Reinhard.estimate`` and
``Reinhard.apply(..., target=)`` (include/stainx_hip.h: sx_reinhard_apply_targets) in LAB, ``ColorDeconvolution.estimate`` and
``ColorDeconvolution.match`` (sx_deconv_moments, sx_deconv_apply) in HED.  The HSV space of the paper is not offered: hue is circular.
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple

import torch
import torch.nn as nn

from stainx_amd import _frontend as fe, masks
from stainx_amd.deconv import ColorDeconvolution, ConcentrationStatistics, check_gain_range
from stainx_amd.normalizers.reinhard import ColorStatistics, Reinhard

SPACES = ("lab", "hed")
KINDS = ("normal", "laplace", "uniform")


class StatisticsDistribution(NamedTuple):
    """The distribution per-tile targets are drawn from: centre and spread of the tiles' channel means, centre and spread of their
    standard deviations -- (3,) float32 each, in the space the statistics were taken in (LAB on the 0..255 scale, or concentrations)."""

    mean_center: torch.Tensor
    mean_spread: torch.Tensor
    std_center: torch.Tensor
    std_spread: torch.Tensor

    @staticmethod
    def fit(*statistics: Any) -> "StatisticsDistribution":
        """From any number of ``ColorStatistics`` / ``(mean, std)`` pairs of (R, 3) rows (a row per tile) and ``ConcentrationStatistics``
        (they enter as ``(s.mean(), s.std())``): the centres are the means of the rows, the spreads their unbiased standard deviations,
        in float64.  Rows that hold a NaN are skipped; fewer than two valid rows is a ValueError.  A one-off call: it copies the rows
        to the host (it may synchronise)."""
        if not statistics:
            raise ValueError("StatisticsDistribution.fit needs at least one set of statistics")
        means, stds = [], []
        for item in statistics:
            if isinstance(item, ConcentrationStatistics):
                mean, std = item._mean_std()
            elif isinstance(item, (tuple, list)) and len(item) == 2:      # (a ColorStatistics is a tuple of two)
                mean, std = item
            else:
                raise ValueError(f"fit takes ColorStatistics, ConcentrationStatistics or (mean, std) pairs, got {type(item).__name__}")
            rows = []
            for name, t in (("mean", mean), ("std", std)):
                if not isinstance(t, torch.Tensor) or not (tuple(t.shape) == (3,) or (t.dim() == 2 and t.shape[1] == 3)):
                    raise ValueError(f"statistics {name} must be a tensor of shape (3,) or (R, 3), got {tuple(getattr(t, 'shape', ()))}")
                rows.append(t.detach().reshape(-1, 3).to("cpu", torch.float64))
            if rows[0].shape[0] != rows[1].shape[0]:
                raise ValueError(f"statistics mean and std must have the same number of rows, got {rows[0].shape[0]} and {rows[1].shape[0]}")
            means.append(rows[0])
            stds.append(rows[1])
        mean, std = torch.cat(means), torch.cat(stds)
        valid = ~(torch.isnan(mean).any(dim=1) | torch.isnan(std).any(dim=1))
        mean, std = mean[valid], std[valid]
        if mean.shape[0] < 2:
            raise ValueError(f"StatisticsDistribution.fit needs at least two rows without NaN, got {mean.shape[0]}")
        return StatisticsDistribution(mean.mean(dim=0).to(torch.float32), mean.std(dim=0, unbiased=True).to(torch.float32),
                                      std.mean(dim=0).to(torch.float32), std.std(dim=0, unbiased=True).to(torch.float32))


def _check_distribution(distribution: Any) -> StatisticsDistribution:
    if not isinstance(distribution, StatisticsDistribution):
        raise ValueError(f"distribution must be a StatisticsDistribution, got {type(distribution).__name__}")
    fields = []
    for name, t in zip(StatisticsDistribution._fields, distribution):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (3,):
            raise ValueError(f"distribution.{name} must be a tensor of shape (3,), got {tuple(getattr(t, 'shape', ()))}")
        fields.append(t.detach().to(torch.float32))
    return StatisticsDistribution(*fields)


class StatisticsAugment(nn.Module):
    """Random per-tile statistics matching of CHW / NCHW tensors on an MI355X (RandStainNA): every tile is moved from its own channel
    statistics to a target drawn from ``distribution``.

    ``space="lab"``: ``Reinhard.estimate`` per tile, then ONE apply launch with a target row per tile (two launches and the statistics
    pass's clearing launch); the target standard deviation is clamped to ``gain_range`` times the tile's own, on the device.  The LAB
    pass keeps the input's element type and scale (uint8 levels, unit floats: ``Reinhard``'s convention) -- ``normalize_to_0_1`` and
    ``basis`` have no say there (no deconvolution is built).  ``space="hed"``: ``ColorDeconvolution(basis).estimate`` (a memset and the moments launch), then ``match`` (one apply
    launch) with ``gain_range``; ``normalize_to_0_1`` as ``HEDAugment``.  ``distribution`` must have been fitted in the same space.

    ``kind``: the law of the draws -- ``"normal"``, ``"laplace"`` or ``"uniform"`` (on [-1, 1]) --, scaled by ``spread_scale`` times
    the distribution's spreads.  ``p``: the probability that a tile is augmented; a tile that is not gets its OWN statistics as target,
    which is the identity up to the apply pass's round trip (LAB and back, or optical density and back) -- not a bit copy.
    ``generator`` drives ``sample_targets`` (drawn on the generator's device, then moved); ``forward(img, targets=(mean, std))`` takes
    explicit targets instead.  ``mask="luminosity"`` (or ``forward(..., mask=tensor)``): statistics over tissue pixels, only they are
    changed.  A tile without statistics (fewer than two pixels or tissue pixels) passes through.  ``device=None`` follows the input
    tensor.  No host synchronisation in ``forward``; all argument errors are raised before any GPU work."""

    def __init__(self, distribution: StatisticsDistribution, space: str = "lab", *, kind: str = "normal", spread_scale: float = 1.0, p: float = 1.0,
                 gain_range: tuple[float, float] = (0.1, 2.5), basis: Any = "hed", generator: torch.Generator | None = None, mask: str | None = None,
                 luminosity_threshold: float = masks.DEFAULT_LUMINOSITY_THRESHOLD, normalize_to_0_1: bool = True, device: str | torch.device | None = None):
        super().__init__()
        self.distribution = _check_distribution(distribution)
        if space not in SPACES:
            raise ValueError(f"space must be one of {list(SPACES)}, got {space!r}")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {list(KINDS)}, got {kind!r}")
        try:
            spread_scale, p = float(spread_scale), float(p)
        except (TypeError, ValueError):
            raise ValueError(f"spread_scale and p must be numbers, got {spread_scale!r} and {p!r}") from None
        if not (math.isfinite(spread_scale) and spread_scale >= 0.0):
            raise ValueError(f"spread_scale must be a finite value >= 0, got {spread_scale}")
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must lie in [0, 1], got {p}")
        self.space, self.kind, self.spread_scale, self.p = space, kind, spread_scale, p
        self.gain_range = check_gain_range(gain_range)
        self.mask = masks.check_mask_mode(mask)
        self.luminosity_threshold = masks.check_threshold(luminosity_threshold)
        self.normalize_to_0_1 = bool(normalize_to_0_1)
        self.generator = generator
        self.device = fe.cuda_only(device, "StatisticsAugment")
        # (`basis` and `normalize_to_0_1` belong to the HED space: the LAB space builds no deconvolution and does not look at them)
        self.deconv = None if space == "lab" else ColorDeconvolution(basis, device=device, normalize_to_0_1=self.normalize_to_0_1, mask=mask,
                                                                     luminosity_threshold=luminosity_threshold)
        self._reinhards: dict[torch.device, Reinhard] = {}
        self._fields: dict[torch.device, StatisticsDistribution] = {}      # (the distribution on a device: uploaded once)

    def _reinhard(self, device: torch.device) -> Reinhard:
        return Reinhard(device=device, backend="torch_hip", statistics="tile", mask=self.mask, luminosity_threshold=self.luminosity_threshold)

    def sample_targets(self, n: int, device: str | torch.device | None = None, *, own: Any = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(target_mean, target_std)``, each (n, 3) float32 on ``device``, drawn with the module's generator (on the generator's
        device, then moved) in a fixed order: ``z`` of shape (2, n, 3) -- ``randn`` (``"normal"``); ``-sign(u) log(1 - 2 |u|)`` with
        ``u = rand - 0.5`` (``"laplace"``; the logarithm's argument is kept at or above the smallest normal float32); ``2 rand - 1``
        (``"uniform"``) --, then ``target_mean = mean_center + spread_scale * mean_spread * z[0]``, ``target_std = std_center +
        spread_scale * std_spread * z[1]``; zero spreads give the centres exactly.  With ``p < 1`` a ``rand(n) < p`` follows: a tile not
        selected gets row t of ``own = (mean, std)`` -- its own statistics, (n, 3) each -- which is then required."""
        device = fe.draw_device(device, self.device)
        if self.p < 1.0:
            if not isinstance(own, (tuple, list)) or len(own) != 2 or any(tuple(getattr(t, "shape", ())) != (n, 3) for t in own):
                raise ValueError(f"sample_targets with p < 1 needs own=(mean, std), the tiles' own statistics of shape ({n}, 3) each")
        if self.kind == "normal":      # (the law is computed where the draw was made, and then moved)
            z = fe.draw(self.generator, (2, n, 3), device, "randn")
        else:
            r = fe.draw(self.generator, (2, n, 3), device)
            if self.kind == "uniform":
                z = 2.0 * r - 1.0
            else:
                u = r - 0.5
                z = -torch.sign(u) * torch.log(torch.clamp(1.0 - 2.0 * torch.abs(u), min=torch.finfo(torch.float32).tiny))
        z = z.to(device)
        held = fe.held(self._fields, device, lambda device: StatisticsDistribution(*(t.to(device) for t in self.distribution)))
        target_mean = held.mean_center + (self.spread_scale * held.mean_spread) * z[0]
        target_std = held.std_center + (self.spread_scale * held.std_spread) * z[1]
        if self.p < 1.0:
            chosen = fe.chosen(self.generator, n, self.p, device)
            target_mean = torch.where(chosen, target_mean, own[0].to(device, torch.float32))
            target_std = torch.where(chosen, target_std, own[1].to(device, torch.float32))
        return target_mean, target_std

    def forward(self, img: torch.Tensor, targets: Any = None, mask: Any = None) -> torch.Tensor:
        """``targets``: an explicit ``(mean, std)`` pair -- (3,), (1, 3) or (N, 3) each, in the module's space -- instead of the draw.
        ``mask``: an explicit uint8 / bool tensor (N, H, W) or (N, 1, H, W) on the device, or ``"luminosity"``, for this call."""
        batch, single, (n, h, w) = fe.image_batch(img, False, "StatisticsAugment")
        if targets is not None:
            targets = fe.mean_std_rows(targets, n, "targets", "ColorStatistics")
        masked, explicit = fe.call_mask(self.mask, mask, single, (n, h, w), self.device or batch.device)
        device = fe.run_device(self.device, batch.device, "StatisticsAugment")
        batch = batch.to(device)
        if self.space == "lab":
            reinhard = fe.held(self._reinhards, device, self._reinhard)
            call_mask = explicit if explicit is not None else ("luminosity" if masked else None)
            own = reinhard.estimate(batch, mask=call_mask)
            if targets is None:
                targets = self.sample_targets(n, device, own=own)
            target_mean, target_std = (t.to(device, torch.float32).reshape(-1, 3).expand(n, 3) for t in targets)
            # (a NaN row of the tile's own statistics makes the target row NaN: the tile is copied either way)
            target_std = torch.minimum(torch.maximum(target_std, self.gain_range[0] * own.std), self.gain_range[1] * own.std)
            out = reinhard.apply(batch, own, mask=call_mask, target=ColorStatistics(target_mean, target_std))
        else:
            if masked and explicit is None:      # (the rule's mask once, for the moments and the apply launch)
                explicit = masks.tissue_mask(batch, self.luminosity_threshold)[0]
            own = self.deconv.estimate(batch, mask=explicit)._mean_std()      # (once: the draw for tiles that are not selected and match read it)
            if targets is None:
                targets = self.sample_targets(n, device, own=own)
            out = self.deconv.match(batch, own, targets, mask=explicit, gain_range=self.gain_range)
        return out.squeeze(0) if single else out

    def extra_repr(self) -> str:
        mask = "None" if self.mask is None else f"{self.mask!r} (luminosity_threshold={self.luminosity_threshold})"
        return (f"space={self.space!r}, kind={self.kind!r}, spread_scale={self.spread_scale}, p={self.p}, gain_range={self.gain_range}, "
                f"normalize_to_0_1={self.normalize_to_0_1}, mask={mask}")
