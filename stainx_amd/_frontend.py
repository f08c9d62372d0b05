"""The rules every public front end shares, each written once: the image preamble, the call's mask, the run device, the per-device caches,
the ``(mean, std)`` pair, the scalar checks and the generator draw.  The front ends -- ``deconv``, ``hsv``, ``augment``,
``statistics_augment``, ``luminosity``, ``masks``, ``focus``, ``sampling`` and the normalisers -- differ in what they call and in the words of
their refusals; the words come in as arguments, the checks are the same.  Everything here runs before any GPU work.  (``masks`` imports
this module and this module imports ``masks``: each uses the other inside functions only.)
"""
from __future__ import annotations

import importlib
from typing import Any, Callable

import torch

from stainx_amd import masks
from stainx_amd.utils import ChannelFormatConverter


# ---------------------------------------------------------------------------------------------------------------------- images
def channels_last(channel_axis: Any) -> bool:
    if channel_axis in ChannelFormatConverter._CHANNELS_LAST:
        return True
    if channel_axis in ChannelFormatConverter._CHANNELS_FIRST:
        return False
    raise ValueError(f"Unsupported channel_axis={channel_axis}")


def _dims(shape: tuple, last: bool) -> tuple[int, int, int]:
    return (shape[0], shape[1], shape[2]) if last else (shape[0], shape[2], shape[3])


def image_batch(x: Any, last: bool, who: str, *, promote: bool = True, tensor: str | None = "a tensor", refusal: str | None = None) -> tuple[Any, bool, tuple[int, int, int]]:
    """``(batch, single, (n, h, w))``: a CHW / HWC tile gains a batch axis (``promote``), the batch is 4-D with C = 3 on the channel axis.
    ``tensor``: how the refusal of a non-tensor names one (None: anything with a ``shape`` is taken, as the normalisers do); ``refusal``: the
    words in front of the shape, where they are not the tile front ends'."""
    if tensor is not None and not isinstance(x, torch.Tensor):
        raise ValueError(f"{who} expects {tensor}, got {type(x).__name__}")
    shape = tuple(getattr(x, "shape", ()))
    single = promote and len(shape) == 3
    if single:
        x, shape = x.unsqueeze(0), (1,) + shape
    if len(shape) != 4 or shape[3 if last else 1] != 3:
        words = refusal or f"{who} expects {'HWC / NHWC' if last else 'CHW / NCHW'} tensors with C=3"
        raise ValueError(f"{words}, got shape {shape}")
    return x, single, _dims(shape, last)


def image_4d(images: Any, channel_axis: Any, who: str) -> tuple[bool, tuple[int, int, int]]:
    """``(channels last?, (n, h, w))`` of the calls that take batches only (``tissue_mask`` and what is documented "as for ``tissue_mask``")."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError(f"{who} expects a 4-D image tensor, got {type(images).__name__} with shape {tuple(getattr(images, 'shape', ()))}")
    last = channels_last(channel_axis)
    if images.shape[-1 if last else 1] != 3:
        raise ValueError(f"{who} expects 3 channels on axis {channel_axis}, got shape {tuple(images.shape)}")
    return last, _dims(images.shape, last)


def tile_mask(mask: Any, single: bool) -> Any:
    """The (H, W) mask of a single tile gains the tile's batch axis; everything else is returned as it is."""
    return mask.unsqueeze(0) if single and isinstance(mask, torch.Tensor) and mask.dim() == 2 else mask


def call_mask(mode: str | None, mask: Any, single: bool, dims: tuple[int, int, int], device: Any, last: bool = False, what: str = "") -> tuple[bool, torch.Tensor | None]:
    """``(masked call?, explicit mask or None)``: ``tile_mask``, then ``masks.resolve`` checks the mask against ``device`` -- the front end's,
    or the tensor's where it has none --, and a masked call on channels-last tiles is refused."""
    masked, explicit = masks.resolve(mode, tile_mask(mask, single), *dims, device)
    if masked and last:
        raise ValueError(f"a masked {what} takes planar (NCHW) tiles only: mask= with channel_axis=-1 is not supported")
    return masked, explicit


# --------------------------------------------------------------------------------------------------------------------- devices
def cuda_only(device: Any, who: str) -> torch.device | None:
    """The constructor's ``device=``: None (follow the tensor) or a CUDA (ROCm) device."""
    device = None if device is None else torch.device(device)
    if device is not None and device.type != "cuda":
        raise ValueError(f"{who} runs on a CUDA (ROCm) device, got {device}")
    return device


def run_device(device: torch.device | None, fallback: torch.device, who: str, got: str = "{} (pass device='cuda' or move the tensor there)") -> torch.device:
    """The device a call runs on: the constructor's or the tensor's; it must be CUDA, and a bare ``cuda`` is the current device."""
    device = torch.device(device) if device is not None else fallback
    if device.type != "cuda":
        raise ValueError(f"{who} runs on a CUDA (ROCm) device; got {got.format(device)}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


ON_TENSOR = "a tensor on {} (pass device='cuda' or move it there)"      # (``run_device``'s ``got`` as MacenkoAugment and LuminosityStandardizer word it)


def held(cache: dict, device: torch.device, make: Callable, *args: Any) -> Any:
    """``cache[device]``, made by ``make(*args, device)`` on first use and kept: an engine (it owns workspaces) or tensors uploaded once (a
    host copy in front of every call would keep the call from being captured).  The dict is the owner's: per instance, or a module's."""
    value = cache.get(device)
    if value is None:
        value = cache[device] = make(*args, device)
    return value


def engine(name: str, device: torch.device) -> Any:
    """A backend class by name, on ``device`` (imported here: importing a front end does not load the native library)."""
    return getattr(importlib.import_module("stainx_amd.backends.torch_hip_backend"), name)(device)


# ----------------------------------------------------------------------------------------------------------- argument checks
def mean_std_rows(pair: Any, n: int, what: str, kind: str, tensors: bool = True) -> tuple[Any, Any]:
    """A ``(mean, std)`` pair, each (3,), (1, 3) or (N, 3) with the same number of rows: checked by shape only."""
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:      # (a ColorStatistics is a tuple of two)
        raise ValueError(f"{what} must be a {kind} or a (mean, std) pair")
    rows = []
    for name, value in zip(("mean", "std"), pair):
        shape = tuple(getattr(value, "shape", ()))
        if (tensors and not isinstance(value, torch.Tensor)) or not (shape == (3,) or (len(shape) == 2 and shape[1] == 3 and shape[0] in (1, n))):
            raise ValueError(f"{what} {name} must {'be a tensor of' if tensors else 'have'} shape (3,), (1, 3) or (N, 3) = ({n}, 3), got {shape}")
        rows.append(1 if len(shape) == 1 else shape[0])
    if rows[0] != rows[1]:
        raise ValueError(f"{what} mean and std must have the same number of rows, got {rows[0]} and {rows[1]}")
    return pair[0], pair[1]


def whole_number(value: Any, rule: str, lo: int | None = None, hi: int | None = None, among: tuple | None = None) -> int:
    """An int -- no bool, no float -- in ``lo..hi`` (either may be open) or ``among`` the given; ``rule`` is the caller's sentence."""
    ok = isinstance(value, int) and not isinstance(value, bool)
    if not ok or (lo is not None and value < lo) or (hi is not None and value > hi) or (among is not None and value not in among):
        raise ValueError(f"{rule}, got {value!r}")
    return value


def real_number(value: Any, unreadable: str, rule: str, accepts: Callable[[float], bool], show: Callable = repr) -> float:
    """``float(value)``: ``unreadable`` where ``float()`` refuses it, ``rule`` where ``accepts(number)`` is false (every comparison with
    a NaN is); both are the caller's sentences.  ``show``: how ``rule`` shows the value (``float``: the number as converted)."""
    try:
        number = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{unreadable}, got {value!r}") from None
    if not accepts(number):
        raise ValueError(f"{rule}, got {show(value)}")
    return number


# ----------------------------------------------------------------------------------------------------------------------- draws
def draw_device(device: Any, own: torch.device | None) -> torch.device:
    """Where ``sample_*`` puts its result: the given device, else the module's, else the CPU."""
    return torch.device(device) if device is not None else (own or torch.device("cpu"))


def draw(generator: torch.Generator | None, shape: tuple, device: torch.device, kind: str = "rand") -> torch.Tensor:
    """float32 ``rand`` / ``randn`` with the module's generator ON THE GENERATOR'S DEVICE (``device`` without one); the caller moves it."""
    return getattr(torch, kind)(shape, generator=generator, device=generator.device if generator is not None else device, dtype=torch.float32)


def draw_seeds(generator: torch.Generator | None, n: int, device: torch.device) -> torch.Tensor:
    """(n,) int64 seeds, ``randint(0, 2^63 - 1)``, under ``draw``'s device rule; the caller moves them."""
    return torch.randint(0, 2**63 - 1, (n,), generator=generator, device=generator.device if generator is not None else device, dtype=torch.int64)


def chosen(generator: torch.Generator | None, n: int, p: float, device: torch.device) -> torch.Tensor:
    """The ``p < 1`` selection, (n, 1) bool on ``device``: one more draw, ``rand(n) < p``."""
    return (draw(generator, (n,), device) < p).to(device).unsqueeze(-1)
