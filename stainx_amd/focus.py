"""Focus measurement: the Laplacian variance and the Tenengrad of tiles, of the cells of a grid on each tile, or of a batch -- the focus
filter that HistoQC-, CLAM- and tiatoolbox-style pipelines run between "find the tissue" and "estimate the stain".  A blurred tile passes
every tissue mask and then feeds a stain estimate as if it were good data.

The scores are ratios of INTEGER sums, and the sums are what the device returns (:class:`FocusStatistics`): exact, independent of the order
of adding, and poolable over batches, slides and ranks (:meth:`FocusStatistics.pool`).  One launch reads a tile once and writes nothing
but the sums; nothing here synchronises, so every call can be captured in a graph.

The rules.  The grey level of a pixel with 8-bit levels r, g, b (the level rule of :func:`stainx_amd.saturation_map`: a uint8 is its own
level, any other type gives ``rint(clip(255 * v, 0, 255))`` in float32): ``Y = (4899 r + 9617 g + 1868 b + 8192) >> 14``, in 0..255 -- the
fixed-point rule of an 8-bit RGB -> grey conversion; a pixel with a NaN in any channel has Y = 0.  On Y, per tile, with the border
reflected without repeating the edge (-1 -> 1, H -> H - 2; an axis of length 1 maps to 0: ``cv2``'s ``BORDER_REFLECT_101``, scipy's
``mode="mirror"``, ``np.pad(mode="reflect")``): ``L = Y[y-1,x] + Y[y+1,x] + Y[y,x-1] + Y[y,x+1] - 4 Y[y,x]`` (``cv2.Laplacian`` with ``ksize=1``)
and the 3 x 3 Sobel responses ``Gx``, ``Gy``, ``T = Gx^2 + Gy^2``.  Tiles never see each other.

NO THRESHOLD IS UNIVERSAL.  The Laplacian variance of sharp tissue depends on the magnification, the scanner, the compression and the
tissue itself: the six 1024 x 1024 images of the test fixture range from 245 to 1170, and a 3 x 3 box blur divides each by 4.9 to 6.4.
Read a threshold from a slide's own distribution::

    stats = sx.focus_statistics(tiles, block=(64, 64), mask="luminosity")
    var = stats.laplacian_variance()                                   # (N, gh, gw) float64, NaN where a cell has no tissue
    enough = stats.pixels >= 1024                                      # cells that are mostly tissue
    cut = 0.25 * var[enough].median()                                  # e.g. a quarter of the slide's typical cell (this line synchronises)
    det = sx.focus_mask(tiles, float(cut), block=(64, 64), mask="luminosity")
    estimate = macenko.estimate(tiles, mask=det.mask)
"""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from stainx_amd import _frontend as fe, masks as _masks

CELL_SIDES = (8, 16, 32, 64)      # include/stainx_hip.h: sx_focus_statistics; and every multiple of 64


class FocusStatistics(NamedTuple):
    """The integer sums behind the focus scores (:func:`focus_statistics` returns it): four int64 tensors of one shape, ``(N, gh, gw)`` -- a
    cell per tile (``gh = gw = 1``) or a grid of cells per tile -- or ``(1, 1, 1)`` pooled over a batch, on the device.  ``pixels``: the pixels
    that entered the cell; ``sums``: sum L (signed); ``squares``: sum L^2; ``gradients``: sum T = sum (Gx^2 + Gy^2)."""

    pixels: torch.Tensor
    sums: torch.Tensor
    squares: torch.Tensor
    gradients: torch.Tensor

    @staticmethod
    def pool(*stats: "FocusStatistics") -> "FocusStatistics":
        """The sum of statistics of equal shapes, integer by integer (a torch add where the tensors live; exact): the same cells seen
        in several batches, on several ranks, or -- after :meth:`total` -- the tiles of a slide."""
        if not stats:
            raise ValueError("pool needs at least one FocusStatistics")
        shape = tuple(stats[0].pixels.shape)
        for item in stats:
            if not isinstance(item, FocusStatistics):
                raise ValueError(f"pool takes FocusStatistics, got {type(item).__name__}")
            if tuple(item.pixels.shape) != shape:
                raise ValueError(f"pool takes statistics of equal shapes, got {shape} and {tuple(item.pixels.shape)}")
        return FocusStatistics(*(torch.stack(list(words)).sum(dim=0) for words in zip(*stats)))

    def total(self) -> "FocusStatistics":
        """The grid of every tile summed to one cell: ``(N, 1, 1)``, equal to the statistics with ``block=None``."""
        return FocusStatistics(*(word.sum(dim=(1, 2), keepdim=True) for word in self))

    def laplacian_variance(self) -> torch.Tensor:
        """``squares / pixels - (sums / pixels)^2`` in float64 on the device (the population variance, ``cv2.Laplacian(gray, CV_64F).var()``);
        NaN where ``pixels == 0``."""
        pixels = self.pixels.to(torch.float64)
        mean = self.sums.to(torch.float64) / pixels
        return self.squares.to(torch.float64) / pixels - mean * mean

    def tenengrad(self) -> torch.Tensor:
        """``gradients / pixels`` in float64 on the device: the mean squared Sobel gradient; NaN where ``pixels == 0``."""
        return self.gradients.to(torch.float64) / self.pixels.to(torch.float64)

    def sharp(self, min_variance: float, *, min_pixels: int = 1) -> torch.Tensor:
        """The cells in focus as a uint8 grid of the statistics' shape: 1 iff ``pixels >= min_pixels`` and the Laplacian variance
        ``>= min_variance`` (a NaN compares false: an empty cell is 0).  Torch ops on the device, no synchronisation."""
        min_variance = _check_variance(min_variance)
        min_pixels = _check_count(min_pixels, "min_pixels")
        return ((self.pixels >= min_pixels) & (self.laplacian_variance() >= min_variance)).to(torch.uint8)


class FocusDetection(NamedTuple):
    """What :func:`focus_mask` returns: ``mask`` (N, H, W) uint8, 1 = a pixel of a sharp cell (and of the tissue mask, if one was given),
    ``counts`` (N,) int64 set pixels per tile and ``statistics``, the :class:`FocusStatistics` of the cells; all on the device."""

    mask: torch.Tensor
    counts: torch.Tensor
    statistics: FocusStatistics


def _check_variance(value: Any) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value:
        raise ValueError(f"min_variance must be a number, got {value!r}")
    return float(value)


def _check_count(value: Any, name: str) -> int:
    return fe.whole_number(value, f"{name} must be a non-negative integer", 0)


def _check_size(value: Any, name: str) -> int:
    return fe.whole_number(value, f"{name} must be a positive integer", 1)


def check_block(block: Any, allow_none: bool = True) -> tuple[int, int] | None:
    """``block=``: None (the whole tile) or ``(bh, bw)``, each side 8, 16, 32, 64 or a multiple of 64."""
    if block is None and allow_none:
        return None
    ok = isinstance(block, (tuple, list)) and len(block) == 2 and all(isinstance(s, int) and not isinstance(s, bool) and (s in CELL_SIDES or (s > 0 and s % 64 == 0)) for s in block)
    if not ok:
        raise ValueError(f"block must be {'None or ' if allow_none else ''}(bh, bw) with each side one of 8, 16, 32, 64 or a multiple of 64, got {block!r}")
    return int(block[0]), int(block[1])


def grey_map(images: torch.Tensor, *, channel_axis: int = 1) -> torch.Tensor:
    """The grey level of a batch: (N, H, W) uint8 on the device, ``Y = (4899 r + 9617 g + 1868 b + 8192) >> 14`` of the pixel's 8-bit levels, one
    streaming kernel (include/stainx_hip.h: sx_grey_map).  ``images`` as for :func:`stainx_amd.tissue_mask`.  A pixel with a NaN in any
    channel has Y = 0.  :func:`stainx_amd.median_filter`, :func:`stainx_amd.level_histogram` and :func:`stainx_amd.level_mask` take the result."""
    last = fe.image_4d(images, channel_axis, "grey_map")[0]
    from stainx_amd.backends.torch_hip_backend import grey_map_native

    return grey_map_native(images, last)


def _statistics(images: torch.Tensor, block: tuple[int, int] | None, mask: Any, pooled: bool, last: bool, dims: tuple[int, int, int],
                threshold: float) -> tuple[FocusStatistics, torch.Tensor | None]:
    from stainx_amd.backends.torch_hip_backend import focus_statistics_native, tissue_mask_native

    if isinstance(mask, torch.Tensor) and images.device.type != "cuda":
        raise ValueError(f"an explicit mask goes with images on the GPU, got images on {images.device}")
    masked, explicit = _masks.resolve(None, mask, *dims, images.device)
    if masked and explicit is None:      # the luminosity rule: the tissue_mask launch in front, on the same stream
        explicit = tissue_mask_native(images, threshold, last)[0]
    words = focus_statistics_native(images, block, explicit, pooled, last)
    return FocusStatistics(words[0], words[1], words[2], words[3]), explicit


def focus_statistics(images: torch.Tensor, *, block: tuple[int, int] | None = None, mask: Any = None, pooled: bool = False, channel_axis: int = 1,
                     luminosity_threshold: float = _masks.DEFAULT_LUMINOSITY_THRESHOLD) -> FocusStatistics:
    """The integer sums of the Laplacian and the Sobel gradient of a batch (module docstring: the rules): :class:`FocusStatistics` of shape
    ``(N, gh, gw)``, or ``(1, 1, 1)`` with ``pooled=True``.  ``images`` as for :func:`stainx_amd.tissue_mask`.

    ``block=None``: a cell per tile.  ``block=(bh, bw)``: a grid of ``ceil(H / bh) x ceil(W / bw)`` cells per tile, edge cells partial; each side
    8, 16, 32, 64 or a multiple of 64.  ``pooled=True`` (with ``block=None`` only): one cell for the batch.  ``mask``: None (every pixel enters its
    cell), ``"luminosity"`` (the :func:`stainx_amd.tissue_mask` launch in front, at ``luminosity_threshold``) or an ``(N, H, W)`` /
    ``(N, 1, H, W)`` uint8 / bool tensor on the images' device; a pixel enters iff its mask byte is non-zero, and its neighbours are read
    whatever the mask says.  One launch (include/stainx_hip.h: sx_focus_statistics, sx_focus_statistics_masked), no workspace, no
    synchronisation."""
    block = check_block(block)
    if pooled and block is not None:
        raise ValueError(f"pooled=True pools whole tiles: it goes with block=None, got block={block!r}")
    threshold = _masks.check_threshold(luminosity_threshold)
    last, dims = fe.image_4d(images, channel_axis, "focus_statistics")
    return _statistics(images, block, mask, bool(pooled), last, dims, threshold)[0]


def cells_mask(cells: torch.Tensor, height: int, width: int, block: tuple[int, int], *, mask: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """A cell grid as a pixel mask: ``(mask, counts)`` -- (N, H, W) uint8, a pixel 1 iff the byte of its cell ``cells[i, y // bh, x // bw]`` is non-zero
    and (``mask`` given) its mask byte is non-zero, and (N,) int64 set pixels per tile, on the device.  ``cells``: (N, ceil(H / bh), ceil(W / bw))
    uint8 / bool on the GPU, what :meth:`FocusStatistics.sharp` returns.  One streaming launch (include/stainx_hip.h: sx_cells_mask)."""
    height, width = _check_size(height, "height"), _check_size(width, "width")
    block = check_block(block, allow_none=False)
    if not isinstance(cells, torch.Tensor) or cells.dtype not in (torch.uint8, torch.bool) or cells.dim() != 3:
        raise ValueError(f"cells must be a uint8 / bool tensor (N, gh, gw), got {type(cells).__name__} {getattr(cells, 'dtype', '')} {tuple(getattr(cells, 'shape', ()))}")
    want = (-(-height // block[0]), -(-width // block[1]))
    if tuple(cells.shape[1:]) != want:
        raise ValueError(f"cells must be (N, gh, gw) with (gh, gw) = {want} for {height} x {width} pixels in {block[0]} x {block[1]} cells, got {tuple(cells.shape)}")
    if cells.device.type != "cuda":
        raise ValueError(f"cells device must be a GPU, got {cells.device}")
    if mask is not None:
        _masks.check_mask_tensor(mask, cells.shape[0], height, width, cells.device)
    from stainx_amd.backends.torch_hip_backend import cells_mask_native

    return cells_mask_native(cells, height, width, block, mask)


def focus_mask(images: torch.Tensor, min_variance: float, *, block: tuple[int, int] = (64, 64), mask: Any = None, min_pixels: int | None = None,
               channel_axis: int = 1, luminosity_threshold: float = _masks.DEFAULT_LUMINOSITY_THRESHOLD) -> FocusDetection:
    """The pixels of the cells in focus: :func:`focus_statistics` on the grid, :meth:`FocusStatistics.sharp` at ``min_variance`` and ``min_pixels``
    (None: a quarter of a full cell), :func:`cells_mask` ANDed with the tissue mask (``mask`` as for :func:`focus_statistics`).  Three launches
    (four with ``mask="luminosity"``) and a few torch ops between them; no synchronisation, so the call can be captured in a graph.
    Every masked call takes the result: ``macenko.estimate(x, mask=det.mask)``, ``sample_pixels(x, ..., mask=det.mask)``.

    No threshold is universal (module docstring): read ``min_variance`` from the slide's own ``laplacian_variance()`` grid."""
    min_variance = _check_variance(min_variance)
    block = check_block(block, allow_none=False)
    min_pixels = (block[0] * block[1]) // 4 if min_pixels is None else _check_count(min_pixels, "min_pixels")
    threshold = _masks.check_threshold(luminosity_threshold)
    last, (n, h, w) = fe.image_4d(images, channel_axis, "focus_mask")
    stats, explicit = _statistics(images, block, mask, False, last, (n, h, w), threshold)
    out, counts = cells_mask(stats.sharp(min_variance, min_pixels=min_pixels), h, w, block, mask=explicit)
    return FocusDetection(out, counts, stats)
