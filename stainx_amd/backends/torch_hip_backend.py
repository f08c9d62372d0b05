"""``backend="torch_hip"``: torch.Tensor in, torch.Tensor out, arithmetic in libstainx_hip.so.

Same class contract as the reference's plugin surface (src/stainx/backends/torch_cuda_backend.py):
``cls(device, **kwargs)`` then ``impl.transform(images, *reference_params)``; exceptions keep the
reference's types (``ImportError`` when the native library is missing, ``ValueError`` for a non-GPU
device or bad shapes, ``RuntimeError`` from the native layer).  Unlike the reference, fit-time
statistics are computed on the device by the same library (reference: always torch on CPU,
torch_backend.py:463-466) -- there is no torch-op or CPU path in this package.

Every rule of the binding is written once.  The shape and dtype rules are the module's pure functions (``_image_shape``,
``_out_flags``, ``_reference_pair``, ``_source_rows``, ``_check_factors``, ``_basis_rows``, ``_hsv_rows``, ``_tone_rows``, ``_tone_seeds``, ``_sigma_rows``, ``_quality_rows``, ``_warp_rows``, ``_elastic_grids``, ``_statistics_rows``,
``_reference_statistics``, ``_explicit_mask``): they take CPU tensors as well, and a tensor moves to the device (``_f32``) after its
check.  The base class holds the image preamble (``_images``), the mask of a masked call (``_mask_for``) and the call rule
(``_call``, under one ``on_device`` guard per public call): the entry point is looked up on ``self._lib``, tensors become their
pointers, ``None`` the null pointer, the current stream comes last, and the status is checked against ``self._lib`` -- the error
string is read from the library that was called.

The order of refusals, for a call with more than one fault: (1) the options that are the method's own (precision, which outputs, scalar
ranges); (2) the images: layout and shape, then the dtype -- also for an empty batch; (3) ``out_dtype``; (4) the reference, then the
other tensor arguments in the order of the signature, a pair's "go together" in front of its shapes; (5) an empty batch returns its
empty result here; (6) an explicit mask.
"""
from __future__ import annotations

import ctypes as _c
import os
import threading

import torch

from stainx_amd import _native

HIP_AVAILABLE = _native.library_available()
_Tensor, _stream_ptr = torch.Tensor, _native.stream_ptr      # (the call rule looks both up once per argument / per call)


# ---- the shape and dtype rules: pure functions, CPU tensors welcome ---------------------------------------------------------------
def _dtype_code(t: torch.Tensor) -> int:
    try:
        return _native.DTYPE_CODES[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported image dtype {t.dtype}; supported: {sorted(str(d) for d in _native.DTYPE_CODES)}") from None


def _image_shape(images: torch.Tensor, channels_last: bool, family: str | None, what: str = "") -> tuple[int, int, int]:
    """``(n, h, w)`` of a batch, NCHW or -- ``channels_last`` -- NHWC.  Anything but four dimensions with three channels is refused in
    the family's words; ``family=None`` (the mask / level functions and luminosity, whose callers have checked) refuses nothing."""
    shape = images.shape
    if family is not None and (len(shape) != 4 or shape[3 if channels_last else 1] != 3):
        shape = tuple(shape)
        if family == "Macenko fit":
            raise ValueError(f"Macenko fit expects NCHW with C=3, got shape {shape}")
        if family == "Macenko":
            if channels_last:
                raise ValueError(f"Macenko {what} with channels_last expects NHWC images with C=3, got shape {shape}")
            if len(shape) != 4:
                raise ValueError(f"Macenko expects NCHW images, got shape {shape}")
            raise ValueError(f"Macenko {what} expects 3 channels in dim 1 (NCHW), got C={shape[1]} with shape {shape}")
        if family == "deconvolution":
            raise ValueError(f"deconvolution {what} expects {'NHWC' if channels_last else 'NCHW'} tensors with 3 channels, got shape {shape}")
        if family in ("HSV", "tone jitter", "Gaussian blur", "JPEG round trip", "affine warp", "elastic warp"):
            raise ValueError(f"{family} {what} expects {'NHWC' if channels_last else 'NCHW'} tensors with 3 channels, got shape {shape}")
        if family == "Reinhard":
            raise ValueError(f"Reinhard expects NCHW images with C=3, got shape {shape}")
        if len(shape) != 4:
            raise ValueError(f"HistogramMatching expects 4D images, got shape {shape}")
        raise ValueError(f"HistogramMatching expects 3 channels, got {shape[-1] if channels_last else shape[1]} with shape {shape}")
    return (shape[0], shape[1], shape[2]) if channels_last else (shape[0], shape[2], shape[3])


def _out_flags(images: torch.Tensor, out_dtype: torch.dtype | None, normalize_to_0_1: bool, channels_last: bool) -> tuple[int, torch.dtype]:
    """The flags and the result's dtype: ``out_dtype`` (an extension, uint8 input only) is bfloat16 / float16 written directly; without
    it the input's dtype, or float32 for the ``/ 255`` of a uint8 batch."""
    flags = (_native.MACENKO_NORMALIZE_0_1 if normalize_to_0_1 else 0) | (_native.MACENKO_CHANNELS_LAST if channels_last else 0)
    if out_dtype is not None and out_dtype != images.dtype:
        if images.dtype != torch.uint8 or out_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"out_dtype is supported for uint8 input and bfloat16 / float16 output, got {images.dtype} -> {out_dtype}")
        return flags | (_native.MACENKO_OUT_BF16 if out_dtype == torch.bfloat16 else _native.MACENKO_OUT_F16), out_dtype
    return flags, torch.float32 if (normalize_to_0_1 and images.dtype == torch.uint8) else images.dtype


def _reference_pair(stain_matrix: torch.Tensor | None, target_max_conc: torch.Tensor | None, together: str | None = None) -> bool:
    """A fitted reference, (3, 2) and 2 values: is one given?  ``together`` is the call's wording of "both or neither"; None: the call
    requires the pair."""
    if together is not None:
        if (stain_matrix is None) != (target_max_conc is None):
            raise ValueError(f"stain_matrix and target_max_conc go together: {together}")
        if stain_matrix is None:
            return False
    if tuple(stain_matrix.shape) != (3, 2):
        raise ValueError(f"stain_matrix must have shape (3, 2), got {stain_matrix.shape}")
    if target_max_conc.numel() != 2:
        raise ValueError(f"target_max_conc must have 2 elements, got {target_max_conc.numel()}")
    return True


def _source_rows(source_he: torch.Tensor, source_max_c: torch.Tensor | None, n: int, need_max_c: bool) -> int:
    """A given source basis, (3, 2), (1, 3, 2) or (N, 3, 2) with 2 values of ``source_max_c`` per row: the number of rows, 1 or N."""
    he_shape = tuple(source_he.shape)
    if he_shape == (3, 2):
        n_sources = 1
    elif len(he_shape) == 3 and he_shape[1:] == (3, 2) and he_shape[0] in (1, n):
        n_sources = he_shape[0]
    else:
        raise ValueError(f"source_he must have shape (3, 2), (1, 3, 2) or (N, 3, 2) = ({n}, 3, 2), got {he_shape}")
    if source_max_c is not None:
        if source_max_c.numel() != 2 * n_sources or (source_max_c.dim() == 2 and tuple(source_max_c.shape) != (n_sources, 2)) or source_max_c.dim() > 2:
            raise ValueError(f"source_max_c must hold 2 values per source basis, ({n_sources}, 2), got shape {tuple(source_max_c.shape)}")
    elif need_max_c:
        raise ValueError("source_max_c is required to normalise to a reference (it may be None in own-basis mode only)")
    return n_sources


def _check_factors(alpha: torch.Tensor, beta: torch.Tensor, n: int, k: int) -> None:
    if tuple(alpha.shape) != (n, k) or tuple(beta.shape) != (n, k):
        raise ValueError(f"alpha and beta must have shape (N, {k}) = ({n}, {k}), got {tuple(alpha.shape)} and {tuple(beta.shape)}")


def _basis_rows(basis: torch.Tensor, n: int, what: str) -> int:
    """A given three-stain basis, (3, 3), (1, 3, 3) or (N, 3, 3): the number of rows, 1 or N."""
    shape = tuple(basis.shape)
    if shape == (3, 3):
        return 1
    if len(shape) == 3 and shape[1:] == (3, 3) and shape[0] in (1, n):
        return shape[0]
    raise ValueError(f"{what} must have shape (3, 3), (1, 3, 3) or (N, 3, 3) = ({n}, 3, 3), got {shape}")


def _hsv_rows(rows: torch.Tensor, n: int) -> int:
    """Rows of an HSV jitter, (5,), (1, 5) or (N, 5): the number of rows, 1 or N."""
    shape = tuple(getattr(rows, "shape", ()))
    if isinstance(rows, torch.Tensor) and shape == (5,):
        return 1
    if isinstance(rows, torch.Tensor) and len(shape) == 2 and shape[1] == 5 and shape[0] in (1, n):
        return shape[0]
    raise ValueError(f"rows must be a tensor of shape (5,), (1, 5) or (N, 5) = ({n}, 5) holding (dh, a_s, b_s, a_v, b_v), got {shape}")


def _sigma_rows(sigmas: torch.Tensor, n: int) -> int:
    """Sigmas of a Gaussian blur, (), (1,) or (N,): the number of rows, 1 or N."""
    shape = tuple(getattr(sigmas, "shape", (-1, -1)))
    if isinstance(sigmas, torch.Tensor) and (shape == () or (len(shape) == 1 and shape[0] in (1, n))):
        return 1 if shape == () else shape[0]
    raise ValueError(f"sigma must be a number or a tensor of shape (), (1,) or (N,) = ({n},), got {shape}")


def _warp_rows(rows: torch.Tensor, n: int) -> int:
    """Rows of an affine warp, (6,), (1, 6) or (N, 6): the number of rows, 1 or N."""
    shape = tuple(getattr(rows, "shape", ()))
    if isinstance(rows, torch.Tensor) and shape == (6,):
        return 1
    if isinstance(rows, torch.Tensor) and len(shape) == 2 and shape[1] == 6 and shape[0] in (1, n):
        return shape[0]
    raise ValueError(f"rows must be a tensor of shape (6,), (1, 6) or (N, 6) = ({n}, 6) holding (a, b, c, d, e, f), got {shape}")


def _elastic_grids(grids: torch.Tensor, n: int, oh: int, ow: int, cell: int) -> int:
    """Control grids of an elastic warp, (2, GH, GW), (1, 2, GH, GW) or (N, 2, GH, GW) for the output size and ``cell``: the number of
    grids, 1 or N."""
    if not isinstance(cell, int) or isinstance(cell, bool) or not _native.ELASTIC_MIN_CELL <= cell <= _native.ELASTIC_MAX_CELL:
        raise ValueError(f"cell must be an int in {_native.ELASTIC_MIN_CELL}..{_native.ELASTIC_MAX_CELL}, got {cell!r}")
    want = (2, (oh - 1) // cell + 4, (ow - 1) // cell + 4)
    shape = tuple(getattr(grids, "shape", ()))
    if isinstance(grids, torch.Tensor) and shape == want:
        return 1
    if isinstance(grids, torch.Tensor) and len(shape) == 4 and shape[1:] == want and shape[0] in (1, n):
        return shape[0]
    raise ValueError(f"grids must be a tensor of shape (2, GH, GW), (1, 2, GH, GW) or (N, 2, GH, GW) = ({n}, {want[0]}, {want[1]}, {want[2]}) for a {oh} x {ow} output at cell {cell}, "
                     f"got {shape if isinstance(grids, torch.Tensor) else type(grids).__name__}")


def _statistics_rows(mean: torch.Tensor, std: torch.Tensor, n: int, what: str, accepted: str = "(3,), (1, 3)") -> tuple[torch.Tensor, torch.Tensor]:
    """Rows of LAB statistics, one for the batch or one per tile, as (rows, 3) tensors.  ``accepted``: the call's wording of the shapes
    it takes beside (N, 3)."""
    if mean.dim() == 1:
        mean = mean.unsqueeze(0)
    if std.dim() == 1:
        std = std.unsqueeze(0)
    for name, t in ((f"{what}_mean", mean), (f"{what}_std", std)):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] not in (1, n):
            raise ValueError(f"{name} must be {accepted} or ({n}, 3) for {n} tiles, got shape {tuple(t.shape)}")
    if mean.shape[0] != std.shape[0]:
        raise ValueError(f"{what}_mean and {what}_std must have the same number of rows, got {mean.shape[0]} and {std.shape[0]}")
    return mean, std


def _reference_statistics(reference_mean: torch.Tensor, reference_std: torch.Tensor) -> None:
    if reference_mean.numel() != 3 or reference_std.numel() != 3:
        raise ValueError("reference_mean / reference_std must have 3 elements")


def _mask_bytes(mask: torch.Tensor | None, device: torch.device) -> torch.Tensor | None:
    """An explicit tissue mask as the dense (N, H, W) uint8 tensor the library reads (bool: the same bytes; no copy where it is dense already)."""
    if mask is None:
        return None
    mask = mask.to(device)
    if mask.dim() == 4:
        mask = mask[:, 0]
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _explicit_mask(mask: torch.Tensor, n: int, h: int, w: int, device: torch.device) -> torch.Tensor:
    """``_mask_bytes`` of an explicit mask that has to be uint8 / bool (N, H, W)."""
    mask = _mask_bytes(mask, device)
    if tuple(mask.shape) != (n, h, w) or mask.dtype != torch.uint8:
        raise ValueError(f"mask must be uint8 / bool (N, H, W) = {(n, h, w)}, got {mask.dtype} {tuple(mask.shape)}")
    return mask


class TorchHIPBackendBase:
    """Common device checks (mirrors TorchCUDABackendBase, torch_cuda_backend.py:17-33), the image preamble and the call rule."""

    def __init__(self, device: str | torch.device | None = None):
        if not _native.library_available():
            _native.require()                      # raises ImportError with the build hint
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("no ROCm device is available on this system")
            self.device = torch.device("cuda", torch.cuda.current_device())
        else:
            self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"HIP backend requires a CUDA (ROCm) device, got {self.device.type}")
        if self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _native.require()
        _native.check_arch(self.device)
        self._scratch = _native.Scratch()

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        # (already float32, contiguous and on the device -- the case of a captured call's fixed buffers, and of every call in a loop --
        # this is the tensor itself; asking first is a third of the time of the two no-op conversions)
        if t.dtype is torch.float32 and t.device == self.device and t.is_contiguous():
            return t
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _images(self, images: torch.Tensor, channels_last: bool, family: str | None, what: str = "") -> tuple[torch.Tensor, int, int, int, int]:
        """The image preamble: the dense batch on the device, ``n, h, w`` and the dtype code, or the family's refusal."""
        if images.device != self.device:
            images = images.to(self.device)
        n, h, w = _image_shape(images, channels_last, family, what)
        code = _native.DTYPE_CODES.get(images.dtype)
        if code is None:
            _dtype_code(images)      # (raises the TypeError)
        return images.contiguous(), n, h, w, code

    def _call(self, name: str, *args, on_failure=None) -> None:
        """The call rule; inside the public call's ``on_device`` guard.  ``on_failure`` runs before a bad status is raised."""
        rc = getattr(self._lib, name)(*[a.data_ptr() if isinstance(a, _Tensor) else a for a in args], _stream_ptr(self.device))
        if rc != 0:
            if on_failure is not None:
                on_failure()
            _native.check(rc, name, self._lib)

    def _check(self, rc: int, what: str) -> None:
        """(the calls that stay written out -- the staged pooled fit, tissue_mask_native -- have their status read here)"""
        if rc != 0:
            _native.check(rc, what, self._lib)

    def _mask_for(self, images: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float) -> torch.Tensor:
        """The dense (N, H, W) uint8 mask a masked call reads: the explicit one, or -- ``mask=None`` -- the luminosity rule's, made by an
        ``sx_tissue_mask`` launch in front of the call on the same stream (one extra streaming pass over the images and its bytes: the
        library's masked Macenko and deconvolution calls take explicit masks only).  ``images``: dense NCHW on the device."""
        n, _, h, w = images.shape
        if mask is not None:
            return _explicit_mask(mask, n, h, w, self.device)
        made = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        self._call("sx_tissue_mask", images, _dtype_code(images), n, h, w, 0, float(luminosity_threshold), made, None)
        return made


# ---- the mask / level functions (stainx_amd.masks, stainx_amd.sampling): their callers have checked the arguments --------------------
def _for_levels(levels: torch.Tensor) -> tuple:
    base = TorchHIPBackendBase(levels.device)
    src = _mask_bytes(levels, base.device)
    return (base, src, *src.shape)


def tissue_mask_native(images: torch.Tensor, luminosity_threshold: float, channels_last: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """``stainx_amd.tissue_mask`` behind its checks: (N, H, W) uint8 mask and (N,) int64 tissue counts (include/stainx_hip.h: sx_tissue_mask)."""
    # (written out: the mask in front of every masked call of the normalisers, and the shared preamble and call rule measured about
    # 1 us of 18 slower here -- profiles/binding_host_time.txt)
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images = images.to(base.device).contiguous()
    n, h, w = (images.shape[0], images.shape[1], images.shape[2]) if channels_last else (images.shape[0], images.shape[2], images.shape[3])
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n == 0 or h * w == 0:
        return mask, counts
    with _native.on_device(base.device):
        rc = base._lib.sx_tissue_mask(images.data_ptr(), _dtype_code(images), n, h, w, int(channels_last), float(luminosity_threshold), mask.data_ptr(),
                                      counts.data_ptr(), _native.stream_ptr(base.device))
    base._check(rc, "sx_tissue_mask")
    return mask, counts


def luminosity_histogram_native(images: torch.Tensor, pooled: bool, channels_last: bool) -> torch.Tensor:
    """``stainx_amd.luminosity_histogram`` behind its checks: (rows, 256) int64 counts on the device (include/stainx_hip.h: sx_luminosity_histogram)."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    counts = torch.zeros((1 if pooled else n, 256), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_luminosity_histogram", images, code, n, h, w, int(channels_last), int(pooled), counts)
    return counts


def tissue_mask_tiles_native(images: torch.Tensor, thresholds: torch.Tensor, channels_last: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """The rule with a threshold per tile (``thresholds``: (N,) float64 on the CPU, each in (0, 1)): (N, H, W) uint8 mask and (N,) int64 counts
    (include/stainx_hip.h: sx_tissue_mask_tiles, with the constants sx_tissue_y_cut gives)."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        cuts = torch.tensor([base._lib.sx_tissue_y_cut(float(t)) for t in thresholds.tolist()], dtype=torch.float32).to(base.device)
        with _native.on_device(base.device):
            base._call("sx_tissue_mask_tiles", images, code, n, h, w, int(channels_last), cuts, mask, counts)
    return mask, counts


def mask_morphology_native(mask: torch.Tensor, op: str, radius: int, element: str) -> tuple[torch.Tensor, torch.Tensor]:
    """``stainx_amd.mask_morphology`` behind its checks: (N, H, W) uint8 result, 1 / 0, and (N,) int64 set pixels per tile (sx_mask_morphology)."""
    base, src, n, h, w = _for_levels(mask)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        scratch = torch.empty_like(out) if op in ("open", "close") else None
        with _native.on_device(base.device):
            base._call("sx_mask_morphology", src, out, n, h, w, _native.MORPH_OPS[op], _native.MORPH_ELEMENTS[element], int(radius), scratch, counts)
    return out, counts


def mask_components_native(mask: torch.Tensor, connectivity: int, holes: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``stainx_amd.mask_components`` behind its checks: (N, H, W) int32 labels and areas, (N,) int64 components per tile (sx_mask_components)."""
    base, src, n, h, w = _for_levels(mask)
    labels = torch.empty((n, h, w), dtype=torch.int32, device=base.device)
    areas = torch.empty((n, h, w), dtype=torch.int32, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_mask_components", src, n, h, w, int(connectivity), int(holes), labels, areas, counts)
    return labels, areas, counts


def mask_area_filter_native(mask: torch.Tensor, min_area: int, connectivity: int, holes: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """``stainx_amd.remove_small_objects`` / ``remove_small_holes`` behind their checks: (N, H, W) uint8 result, 1 / 0, and (N,) int64 set pixels per
    tile (sx_mask_area_filter; the workspace comes from its size query)."""
    base, src, n, h, w = _for_levels(mask)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        workspace = torch.empty((int(base._lib.sx_mask_components_workspace_bytes(n, h, w)),), dtype=torch.uint8, device=base.device)
        with _native.on_device(base.device):
            base._call("sx_mask_area_filter", src, out, n, h, w, int(connectivity), int(holes), int(min_area), workspace, counts)
    return out, counts


def saturation_map_native(images: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """``stainx_amd.saturation_map`` behind its checks: (N, H, W) uint8 saturation levels on the device (include/stainx_hip.h: sx_saturation_map)."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_saturation_map", images, code, n, h, w, int(channels_last), out)
    return out


def grey_map_native(images: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """``stainx_amd.grey_map`` behind its checks: (N, H, W) uint8 grey levels on the device (include/stainx_hip.h: sx_grey_map)."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_grey_map", images, code, n, h, w, int(channels_last), out)
    return out


def focus_statistics_native(images: torch.Tensor, block: tuple[int, int] | None, mask: torch.Tensor | None, pooled: bool, channels_last: bool) -> torch.Tensor:
    """``stainx_amd.focus_statistics`` behind its checks: (4, N, gh, gw) int64 -- pixels, sum L, sum L^2, sum T -- on the device, (4, 1, 1, 1) pooled
    (include/stainx_hip.h: sx_focus_statistics, sx_focus_statistics_masked).  ``mask``: None or an explicit (N, H, W) uint8 / bool tensor."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    bh, bw = block if block is not None else (0, 0)
    cells = (1, 1, 1) if pooled else (n, -(-h // bh) if bh else 1, -(-w // bw) if bw else 1)
    if n * h * w == 0:
        return torch.zeros((4, *cells), dtype=torch.int64, device=base.device)
    out = torch.empty((4, *cells), dtype=torch.int64, device=base.device)      # (the library clears what it adds into)
    with _native.on_device(base.device):
        if mask is None:
            base._call("sx_focus_statistics", images, code, n, h, w, int(channels_last), bh, bw, int(pooled), out)
        else:
            base._call("sx_focus_statistics_masked", images, code, n, h, w, int(channels_last), bh, bw, int(pooled), _explicit_mask(mask, n, h, w, base.device), out)
    return out


def cells_mask_native(cells: torch.Tensor, height: int, width: int, block: tuple[int, int], mask: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
    """``stainx_amd.cells_mask`` behind its checks: (N, H, W) uint8 mask, 1 / 0, and (N,) int64 set pixels per tile (sx_cells_mask)."""
    base, src, n, _, _ = _for_levels(cells)
    out = torch.empty((n, height, width), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device) if n * height * width == 0 else torch.empty((n,), dtype=torch.int64, device=base.device)
    if n * height * width != 0:
        given = None if mask is None else _explicit_mask(mask, n, height, width, base.device)
        with _native.on_device(base.device):
            base._call("sx_cells_mask", src, n, height, width, int(block[0]), int(block[1]), given, out, counts)
    return out, counts


def median_filter_native(levels: torch.Tensor, size: int) -> torch.Tensor:
    """``stainx_amd.median_filter`` behind its checks: (N, H, W) uint8 medians of the size x size windows (sx_median_filter_u8)."""
    base, src, n, h, w = _for_levels(levels)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_median_filter_u8", src, out, n, h, w, int(size))
    return out


def level_histogram_native(levels: torch.Tensor, pooled: bool) -> torch.Tensor:
    """``stainx_amd.level_histogram`` behind its checks: (rows, 256) int64 counts on the device (sx_level_histogram)."""
    base, src, n, h, w = _for_levels(levels)
    counts = torch.zeros((1 if pooled else n, 256), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_level_histogram", src, n, h, w, int(pooled), counts)
    return counts


def level_mask_native(levels: torch.Tensor, thresholds: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``stainx_amd.level_mask`` behind its checks (``thresholds``: (N,) int32 on the device): (N, H, W) uint8 mask, 1 where level > threshold, and
    (N,) int64 set pixels per tile (sx_level_mask_tiles)."""
    base, src, n, h, w = _for_levels(levels)
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=base.device)
    counts = torch.zeros((n,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        with _native.on_device(base.device):
            base._call("sx_level_mask_tiles", src, n, h, w, thresholds, mask, counts)
    return mask, counts


def sample_pixels_native(images: torch.Tensor, mask: torch.Tensor | None, height: int, width: int, pooled: bool, offset: int,
                         channels_last: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``stainx_amd.sample_pixels`` behind its checks (``mask``: an explicit mask or None, every pixel): (G, 3, height, width) pixels of the images'
    type, (G, height, width) uint8 validity, (G,) int32 taken and (G,) int64 population, G = 1 pooled, else N (include/stainx_hip.h:
    sx_sample_pixels; the workspace comes from its size query).  Nothing synchronises."""
    base = TorchHIPBackendBase(images.device if images.device.type == "cuda" else None)
    images, n, h, w, code = base._images(images, channels_last, None)
    groups = 1 if pooled else n
    make = torch.zeros if n * h * w == 0 else torch.empty      # nothing to rank: empty groups (a pooled call keeps its one row)
    pixels = make((groups, 3, height, width), dtype=images.dtype, device=base.device)
    valid = make((groups, height, width), dtype=torch.uint8, device=base.device)
    taken = make((groups,), dtype=torch.int32, device=base.device)
    population = make((groups,), dtype=torch.int64, device=base.device)
    if n * h * w != 0:
        src = _mask_bytes(mask, base.device)
        nbytes = int(base._lib.sx_sample_workspace_bytes(n, h, w))
        if nbytes == 0:
            raise ValueError(f"sample_pixels: a tile of {h} x {w} pixels is too large for one call (a group holds fewer than 2^31 pixels)")
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=base.device)
        with _native.on_device(base.device):
            base._call("sx_sample_pixels", images, code, n, h, w, int(channels_last), src, int(pooled), height * width, int(offset), pixels, valid, taken, population, workspace, nbytes)
    return pixels, valid, taken, population


class MacenkoHIP(TorchHIPBackendBase):
    """Macenko transform / fit on the GPU (numerics of MacenkoTorch, torch_backend.py:358-560)."""

    def __init__(self, device: str | torch.device | None = None, precision: str = "stable", diag: bool = False):
        super().__init__(device)
        if diag:      # tests / tools: the diagnostic build (its flags force the rare paths; the design-study forms live there)
            self._lib = _native.require_diag()
        if precision not in ("stable", "fast", "sampled"):
            raise ValueError(f"precision must be 'stable' or 'fast' (or the extension 'sampled'), got {precision!r}")
        # "stable" and "fast" run the SAME exact kernels (fp64 covariance, exact nearest-rank percentiles).  The reference's "fast"
        # (torch_cuda_backend.py:114-118; macenko.cu:116-191) keeps the exact percentiles and moves the big tensors to fp16 for a
        # 1.2-1.3x gain at MAE ~0.05 grey levels; here the exact path is the fast one, and its result lies inside that mode's
        # tolerance (tests/test_precision_modes_gpu.py holds it to the restated fp16 path).
        # "sampled" (an extension, opt-in, NOT a parity path): the percentiles of a 4096-pixel sample of each tile stand in for the
        # exact ones -- moments pass + one per-tile stage + reconstruct; mean error ~0.5, worst ~5 grey levels.  The fit is always exact.
        self._precision = precision
        self.last_workspace: torch.Tensor | None = None
        self._pfit_bytes: dict[tuple[int, int, int], int] = {}
        # Feedback for the choice between the two forms of the transform (see _route / _watch): the two-pass form speculates per
        # tile and pays a whole-tile exact select (0.1-0.5 ms) for a tile it cannot speculate on -- no tissue, no stable stain
        # plane.  The library counts those; the count is read back asynchronously and a batch stream that produces them is
        # switched to the four-pass form (same bits, no cliff), with an occasional probe.
        self._tele_offset = int(self._lib.sx_macenko_telemetry_offset())
        self._tele_host: torch.Tensor | None = None
        self._tele_event: torch.cuda.Event | None = None
        self._tele_stream: torch.cuda.Stream | None = None
        self._classic_left = 0
        self._classic_span = 32
        self._tele_age = 0
        self._tele_ptr = 0
        self._tele_seen: dict[int, tuple[int, int]] = {}      # workspace pointer -> (slow selections, waits that ran out) read there last
        self._tele_lock = threading.Lock()                     # (one object may be driven from several threads, each on its own stream)
        # A/B switch for benchmarks (it used to live inside the library): the four-pass form everywhere
        self._env_flags = _native.MACENKO_CLASSIC if os.environ.get("STAINX_MACENKO_CLASSIC", "").strip().lower() in ("1", "true", "yes", "on") else 0

    def _reference(self, stain_matrix, target_max_conc, together: str | None = None) -> tuple[torch.Tensor | None, torch.Tensor | None]:
        """The fitted reference as float32 device tensors, (3, 2) and (2,), or ``(None, None)`` where the call may do without."""
        if not _reference_pair(stain_matrix, target_max_conc, together):
            return None, None
        return self._f32(stain_matrix), self._f32(target_max_conc).flatten()

    def _check_sources(self, source_he: torch.Tensor, source_max_c: torch.Tensor | None, n: int, need_max_c: bool) -> tuple[torch.Tensor, torch.Tensor | None, int]:
        """A given source basis as float32 device tensors, and the number of its rows, 1 or N."""
        n_sources = _source_rows(source_he, source_max_c, n, need_max_c)
        return self._f32(source_he), None if source_max_c is None else self._f32(source_max_c), n_sources

    def _masked_images(self, images: torch.Tensor, what: str) -> tuple[torch.Tensor, int, int, int, int]:
        if self._precision == "sampled":
            raise ValueError(f"{what} with a mask runs the exact four-pass form; precision='sampled' has no masked form")
        return self._images(images, False, "Macenko", what)

    def _classic_workspace(self, code: int, n: int, h: int, w: int) -> torch.Tensor:
        return self._scratch.get(self._lib.sx_macenko_workspace_bytes_for(code, n, h, w, _native.MACENKO_CLASSIC), self.device)

    def transform(self, images: torch.Tensor, stain_matrix: torch.Tensor, target_max_conc: torch.Tensor, *, normalize_to_0_1: bool = False,
                  channels_last: bool = False, out_dtype: torch.dtype | None = None, _extra_flags: int = 0) -> torch.Tensor:
        """``channels_last=True`` (an extension; the reference takes NCHW only): ``images`` is (N,H,W,3) as decoders and PIL
        hand tiles over, and so is the result -- the permute + copy a caller would otherwise do first is fused away.
        ``out_dtype=torch.bfloat16 / torch.float16`` (an extension, uint8 input only): the result of the call without it, cast
        with ``.to(out_dtype)``, written directly -- a decoder's uint8 tile becomes a model's half-precision input in one call."""
        images, n, h, w, code = self._images(images, channels_last, "Macenko", "transform")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        sm, tmc = self._reference(stain_matrix, target_max_conc)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            flags |= (_native.MACENKO_SAMPLED if self._precision == "sampled" else 0) | int(_extra_flags) | self._env_flags
            # (only calls the library would run in its two-pass form take part in the feedback: for the others -- small batches,
            # narrow pixels -- the event, the side-stream copy and the stream bookkeeping are 7 us of host time per call for nothing)
            routed = (not (flags & (_native.MACENKO_CLASSIC | _native.MACENKO_TWO_PASS | _native.MACENKO_SAMPLED))
                      and self._lib.sx_macenko_takes_two_pass(code, n, h, w, flags) == 1)
            # the workspace of the form the library WOULD take: a routed call may be sent to the four-pass form below, whose
            # workspace is a prefix of it (one buffer per stream serves both)
            nbytes = self._lib.sx_macenko_workspace_bytes_for(code, n, h, w, flags)
            ws = self._scratch.get(nbytes, self.device)
            if routed:
                with self._tele_lock:
                    flags |= self._route()
            self._call("sx_macenko_transform", images, out, code, n, h, w, sm, tmc, flags, ws, ws.numel())
            if routed and not (flags & _native.MACENKO_CLASSIC):
                with self._tele_lock:
                    self._watch(ws)
        self.last_workspace = ws
        return out

    def augment(self, images: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, stain_matrix: torch.Tensor | None = None,
                target_max_conc: torch.Tensor | None = None, *, normalize_to_0_1: bool = False, channels_last: bool = False,
                out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """Stain augmentation (an extension; include/stainx_hip.h: sx_macenko_augment): every tile's H and E concentrations, in
        the tile's own stain basis, become ``alpha * C + beta`` (``alpha``, ``beta``: (N, 2) per tile, (H, E)) and the tile is
        rebuilt -- with its own ``HE_source`` when no reference is given, with the fitted ``stain_matrix`` after the transform's
        rescaling ``C * target_max_conc / maxC`` otherwise.  Images, layout and output types as in ``transform``.  The factors are
        read on the device: a captured call replayed after new values are copied into the same tensors uses the new values."""
        return self._augment_call(self._images(images, channels_last, "Macenko", "augment"), alpha, beta, stain_matrix, target_max_conc, None, normalize_to_0_1, channels_last, out_dtype)

    def _augment_call(self, batch: tuple, alpha, beta, stain_matrix, target_max_conc, masking: tuple | None, normalize_to_0_1: bool, channels_last: bool, out_dtype) -> torch.Tensor:
        """augment / augment_masked: ``masking`` is None or ``(mask, luminosity_threshold)``."""
        images, n, h, w, code = batch
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        sm, tmc = self._reference(stain_matrix, target_max_conc, "both (normalise and jitter) or neither (each tile's own stain basis)")
        _check_factors(alpha, beta, n, 2)
        a, b = self._f32(alpha), self._f32(beta)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = None if masking is None else self._mask_for(images, *masking)
            ws = self._classic_workspace(code, n, h, w)
            if masking is None:
                self._call("sx_macenko_augment", images, out, code, n, h, w, a, b, sm, tmc, flags, ws, ws.numel())
            else:
                self._call("sx_macenko_augment_masked", images, out, code, n, h, w, mask, a, b, sm, tmc, flags, ws, ws.numel())
        self.last_workspace = ws
        return out

    def separate(self, images: torch.Tensor, stain_matrix: torch.Tensor | None = None, target_max_conc: torch.Tensor | None = None, *,
                 stains: bool = True, concentrations: bool = False, max_conc: bool = False, normalize_to_0_1: bool = False,
                 channels_last: bool = False, out_dtype: torch.dtype | None = None) -> dict[str, torch.Tensor | None]:
        """Stain separation (include/stainx_hip.h: sx_macenko_separate): every tile's H and E concentrations ``C = pinv(HE_source) OD``
        (the transform's per-tile estimate), in the tile's own basis when no reference is given, normalised ``C * target_max_conc /
        maxC`` with a fitted reference.  Returns ``stains`` (2, N, 3, H, W) -- the H images, then the E images, built with the tile's
        ``HE_source`` or the reference's ``stain_matrix`` and typed as ``transform`` types its output --, ``concentrations`` (N, 2, H, W)
        float32, ``he`` (N, 3, 2) and ``max_c`` (N, 2); an output not asked for is None.  ``max_c`` comes with normalised mode for free;
        in own-basis mode ``max_conc=True`` adds the two launches that compute it.  ``channels_last``: NHWC images, (2, N, H, W, 3)
        images and (N, H, W, 2) concentrations."""
        return self._separate_call(images, stain_matrix, target_max_conc, source=None, masking=None, stains=stains, concentrations=concentrations, max_conc=max_conc,
                                   normalize_to_0_1=normalize_to_0_1, channels_last=channels_last, out_dtype=out_dtype, neither="each tile's own stain basis")

    def estimate(self, images: torch.Tensor, *, channels_last: bool = False) -> dict[str, torch.Tensor]:
        """The transform's per-tile estimate as a call of its own (include/stainx_hip.h: sx_macenko_estimate): ``he`` (N, 3, 2),
        ``max_c`` (N, 2) and ``tissue`` (N,) -- the pixels the optical-density filter kept -- of every tile; no output pass.  Always
        the exact percentiles: ``precision="sampled"`` is refused."""
        if self._precision == "sampled":
            raise ValueError("estimate computes the exact per-tile estimate; precision='sampled' has no estimate of its own")
        images, n, h, w, code = self._images(images, channels_last, "Macenko", "estimate")
        out = {
            "he": torch.empty((n, 3, 2), dtype=torch.float32, device=self.device),
            "max_c": torch.empty((n, 2), dtype=torch.float32, device=self.device),
            "tissue": torch.empty((n,), dtype=torch.float32, device=self.device),
        }
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            ws = self._classic_workspace(code, n, h, w)
            self._call("sx_macenko_estimate", images, code, n, h, w, out["he"], out["max_c"], out["tissue"], _native.MACENKO_CHANNELS_LAST if channels_last else 0, ws, ws.numel())
        self.last_workspace = ws
        return out

    def apply(self, images: torch.Tensor, source_he: torch.Tensor, source_max_c: torch.Tensor | None, stain_matrix: torch.Tensor | None = None,
              target_max_conc: torch.Tensor | None = None, *, alpha: torch.Tensor | None = None, beta: torch.Tensor | None = None,
              normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False, _masking: tuple | None = None) -> torch.Tensor:
        """Normalise (and optionally jitter) with a GIVEN source basis (include/stainx_hip.h: sx_macenko_apply): one kernel launch, no
        estimate, no workspace, no host synchronisation.  ``source_he`` is (3, 2) or (1, 3, 2) -- one basis for the batch -- or
        (N, 3, 2), ``source_max_c`` (2,), (1, 2) or (N, 2) to match.  With ``stain_matrix`` / ``target_max_conc`` the tiles are
        normalised to that reference, ``alpha`` / ``beta`` (N, 2) jitter the concentrations on top; without a reference (own basis)
        the factors are required, the tile is rebuilt with ``source_he`` and ``source_max_c`` is not read (it may be None).  Images,
        layout and output types as in ``transform``.  Source, factors and reference are read on the device: a captured call replayed
        after new values are copied into the same tensors uses the new values."""
        images, n, h, w, code = self._images(images, channels_last, "Macenko", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        sm, tmc = self._reference(stain_matrix, target_max_conc, "both (normalise) or neither (the given source basis is kept)")
        if (alpha is None) != (beta is None):
            raise ValueError("alpha and beta go together: both or neither")
        if sm is None and alpha is None:
            raise ValueError("apply without a reference (own basis) needs the factors alpha and beta")
        he, mc, n_sources = self._check_sources(source_he, source_max_c, n, sm is not None)
        a = b = None
        if alpha is not None:
            _check_factors(alpha, beta, n, 2)
            a, b = self._f32(alpha), self._f32(beta)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if _masking is None:
                self._call("sx_macenko_apply", images, out, code, n, h, w, he, mc, n_sources, a, b, sm, tmc, flags)
            else:      # (apply_masked: the same arguments and one more; the rule's mask is a launch of its own in front)
                self._call("sx_macenko_apply_masked", images, out, code, n, h, w, he, mc, n_sources, a, b, sm, tmc, self._mask_for(images, *_masking), flags)
        return out

    # ---- tissue masks (include/stainx_hip.h: sx_macenko_*_masked): the estimate over the masked-in pixels, masked-out pixels copied ----
    def estimate_masked(self, images: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float = 0.8, *, pooled: bool = False) -> dict[str, torch.Tensor]:
        """``estimate`` over the masked-in pixels only (``mask``: (N, H, W) uint8 / bool, or None: the luminosity rule): ``he`` (rows, 3, 2),
        ``max_c`` (rows, 2), ``tissue`` (rows,) float32 -- the pixels of the selection set -- and ``mask_pixels`` (rows,) int64, the exact
        masked-in counts; rows = N, or 1 with ``pooled`` (one estimate over the masked-in pixels of the batch, the pooled fit's path).  A
        group without an estimate (per tile: fewer than 3 masked-in pixels; pooled: fewer than 3 that also pass the OD filter) has NaN
        rows and ``tissue`` 0."""
        images, n, h, w, code = self._masked_images(images, "estimate")
        rows = 1 if pooled else n
        out = {
            "he": torch.empty((rows, 3, 2), dtype=torch.float32, device=self.device),
            "max_c": torch.empty((rows, 2), dtype=torch.float32, device=self.device),
            "tissue": torch.empty((rows,), dtype=torch.float32, device=self.device),
            "mask_pixels": torch.empty((rows,), dtype=torch.int64, device=self.device),
        }
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = self._mask_for(images, mask, luminosity_threshold)
            ws = self._classic_workspace(code, n, h, w)
            self._call("sx_macenko_estimate_masked", images, code, n, h, w, mask, int(pooled), out["he"], out["max_c"], out["tissue"], out["mask_pixels"], 0, ws, ws.numel())
        self.last_workspace = ws
        return out

    def compute_reference_stain_matrix_masked(self, images: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float = 0.8) -> tuple[torch.Tensor, torch.Tensor]:
        """The pooled fit over the masked-in pixels of the batch: ``(HE (3,2), maxC (2,))``; NaN when fewer than 3 of them pass the OD filter."""
        out = self.estimate_masked(images, mask, luminosity_threshold, pooled=True)
        return out["he"][0], out["max_c"][0]

    def transform_masked(self, images: torch.Tensor, stain_matrix: torch.Tensor, target_max_conc: torch.Tensor, mask: torch.Tensor | None,
                         luminosity_threshold: float = 0.8, *, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, _extra_flags: int = 0) -> torch.Tensor:
        """``transform`` with a tissue mask: the per-tile estimate over the masked-in pixels, those pixels normalised with it, the others
        (and tiles without an estimate) copied.  Always the four-pass form: no routing, no telemetry, no host synchronisation."""
        images, n, h, w, code = self._masked_images(images, "transform")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, False)
        sm, tmc = self._reference(stain_matrix, target_max_conc)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = self._mask_for(images, mask, luminosity_threshold)
            ws = self._classic_workspace(code, n, h, w)
            self._call("sx_macenko_transform_masked", images, out, code, n, h, w, mask, sm, tmc, flags | int(_extra_flags), ws, ws.numel())
        self.last_workspace = ws
        return out

    def apply_masked(self, images: torch.Tensor, source_he: torch.Tensor, source_max_c: torch.Tensor | None, stain_matrix: torch.Tensor | None,
                     target_max_conc: torch.Tensor | None, mask: torch.Tensor | None, luminosity_threshold: float = 0.8, *, alpha: torch.Tensor | None = None,
                     beta: torch.Tensor | None = None, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """``apply`` with a tissue mask (all its modes): still one launch for an explicit mask; masked-out pixels, and tiles whose source row
        holds a NaN, are copied."""
        images = self._masked_images(images, "apply")[0]
        return self.apply(images, source_he, source_max_c, stain_matrix, target_max_conc, alpha=alpha, beta=beta, normalize_to_0_1=normalize_to_0_1,
                          out_dtype=out_dtype, _masking=(mask, luminosity_threshold))

    # ---- separation / augmentation with a given source basis and under tissue masks (include/stainx_hip.h) ----
    def _separate_call(self, images: torch.Tensor, stain_matrix, target_max_conc, *, source, masking, stains: bool, concentrations: bool, max_conc: bool,
                       normalize_to_0_1: bool, channels_last: bool, out_dtype, neither: str = "the source basis itself") -> dict[str, torch.Tensor | None]:
        """separate / separate_apply / separate_apply_masked / separate_masked: ``source`` is None (the call's own estimate) or
        ``(source_he, source_max_c)``; ``masking`` is None or ``(mask, luminosity_threshold)``."""
        if not (stains or concentrations):
            raise ValueError("separate: ask for stains, concentrations or both")
        images, n, h, w, code = self._images(images, channels_last, "Macenko", "separate") if masking is None else self._masked_images(images, "separate")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        sm, tmc = self._reference(stain_matrix, target_max_conc, f"both (normalised) or neither ({neither})")
        he = mc = None
        n_sources = n
        if source is not None:
            he, mc, n_sources = self._check_sources(source[0], source[1], n, sm is not None)
        out = {
            "stains": torch.empty((2, *images.shape), dtype=out_dtype, device=self.device) if stains else None,
            "concentrations": torch.empty((n, h, w, 2) if channels_last else (n, 2, h, w), dtype=torch.float32, device=self.device) if concentrations else None,
        }
        if source is not None:      # (the given rows, broadcast to N)
            out["he"] = he.reshape(n_sources, 3, 2).expand(n, 3, 2)
            out["max_c"] = mc.reshape(n_sources, 2).expand(n, 2) if mc is not None else None
        else:
            out["he"] = torch.empty((n, 3, 2), dtype=torch.float32, device=self.device)
            out["max_c"] = torch.empty((n, 2), dtype=torch.float32, device=self.device) if (max_conc or sm is not None) else None
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = self._mask_for(images, *masking) if masking is not None else None
            if source is None:
                ws = self._classic_workspace(code, n, h, w)
                if mask is None:
                    self._call("sx_macenko_separate", images, out["stains"], out["concentrations"], code, n, h, w, sm, tmc, out["he"], out["max_c"], flags, ws, ws.numel())
                else:
                    self._call("sx_macenko_separate_masked", images, out["stains"], out["concentrations"], code, n, h, w, mask, sm, tmc, out["he"], out["max_c"], flags, ws, ws.numel())
                self.last_workspace = ws
            elif mask is None:
                self._call("sx_macenko_separate_apply", images, out["stains"], out["concentrations"], code, n, h, w, he, mc, n_sources, sm, tmc, flags)
            else:
                self._call("sx_macenko_separate_apply_masked", images, out["stains"], out["concentrations"], code, n, h, w, he, mc, n_sources, sm, tmc, mask, flags)
        return out

    def separate_apply(self, images: torch.Tensor, source_he: torch.Tensor, source_max_c: torch.Tensor | None, stain_matrix: torch.Tensor | None = None,
                       target_max_conc: torch.Tensor | None = None, *, stains: bool = True, concentrations: bool = False, normalize_to_0_1: bool = False,
                       channels_last: bool = False, out_dtype: torch.dtype | None = None) -> dict[str, torch.Tensor | None]:
        """``separate`` with a GIVEN source basis (include/stainx_hip.h: sx_macenko_separate_apply): one kernel launch, no estimate, no
        workspace, no host synchronisation.  ``source_he`` / ``source_max_c`` as ``apply`` takes them (one row or N; ``source_max_c`` may
        be None in own basis).  Returns ``separate``'s dictionary; ``he`` / ``max_c`` are the given rows broadcast to N."""
        return self._separate_call(images, stain_matrix, target_max_conc, source=(source_he, source_max_c), masking=None, stains=stains, concentrations=concentrations,
                                   max_conc=False, normalize_to_0_1=normalize_to_0_1, channels_last=channels_last, out_dtype=out_dtype)

    def separate_apply_masked(self, images: torch.Tensor, source_he: torch.Tensor, source_max_c: torch.Tensor | None, stain_matrix: torch.Tensor | None,
                              target_max_conc: torch.Tensor | None, mask: torch.Tensor | None, luminosity_threshold: float = 0.8, *, stains: bool = True,
                              concentrations: bool = False, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None) -> dict[str, torch.Tensor | None]:
        """``separate_apply`` with a tissue mask (``mask=None``: the luminosity rule, one launch in front): masked-out pixels, and tiles
        whose source row holds a NaN, hold no stain -- concentrations +0, stain images the 240 level."""
        return self._separate_call(images, stain_matrix, target_max_conc, source=(source_he, source_max_c), masking=(mask, luminosity_threshold), stains=stains,
                                   concentrations=concentrations, max_conc=False, normalize_to_0_1=normalize_to_0_1, channels_last=False, out_dtype=out_dtype)

    def separate_masked(self, images: torch.Tensor, stain_matrix: torch.Tensor | None, target_max_conc: torch.Tensor | None, mask: torch.Tensor | None,
                        luminosity_threshold: float = 0.8, *, stains: bool = True, concentrations: bool = False, max_conc: bool = False, normalize_to_0_1: bool = False,
                        out_dtype: torch.dtype | None = None) -> dict[str, torch.Tensor | None]:
        """``separate`` with a tissue mask: the per-tile estimate over the masked-in pixels, then the masked separation pass.  A tile
        without an estimate (fewer than 3 masked-in pixels) has NaN ``he`` / ``max_c`` rows and comes out entirely as background."""
        return self._separate_call(images, stain_matrix, target_max_conc, source=None, masking=(mask, luminosity_threshold), stains=stains, concentrations=concentrations,
                                   max_conc=max_conc, normalize_to_0_1=normalize_to_0_1, channels_last=False, out_dtype=out_dtype)

    def augment_masked(self, images: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, stain_matrix: torch.Tensor | None, target_max_conc: torch.Tensor | None,
                       mask: torch.Tensor | None, luminosity_threshold: float = 0.8, *, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None) -> torch.Tensor:
        """``augment`` with a tissue mask: the per-tile estimate over the masked-in pixels, the jitter on those pixels; masked-out pixels,
        and tiles without an estimate, are copied by ``transform_masked``'s background rule."""
        return self._augment_call(self._masked_images(images, "augment"), alpha, beta, stain_matrix, target_max_conc, (mask, luminosity_threshold), normalize_to_0_1, False, out_dtype)

    def _route(self) -> int:
        """Flag for this call: the four-pass form while a recent call reported tiles the two-pass form could not speculate on.
        Never synchronises the host with the device except to wait for an answer that is five calls old (see below)."""
        if torch.cuda.is_current_stream_capturing():
            return _native.MACENKO_CLASSIC      # a captured call is replayed on data nobody has seen: the form without a cliff (and no event may be queried here)
        if self._tele_event is not None:
            self._tele_age += 1
            if self._tele_age > 4 and not self._tele_event.query():
                # The host runs ahead of the device (a loop that never synchronises queues its calls long before they run): an
                # answer that is five calls old is waited for, so that a batch the two-pass form cannot speculate on costs a few
                # slow calls, not every call until the host happens to synchronise.  Five calls are still queued behind the one
                # waited for: the device does not run dry.
                self._tele_event.synchronize()
        if self._tele_event is not None and self._tele_event.query():
            # running counts (the library only adds to them): what is new since the last look at THIS workspace.  The first look
            # at a workspace only sets its base (fresh memory holds anything) -- taken from this same asynchronous read-back, so
            # a call on a new stream or a grown scratch costs no host synchronisation.
            now = (int(self._tele_host[0]) & 0xFFFFFFFF, int(self._tele_host[1]) & 0xFFFFFFFF)
            seen = self._tele_seen.get(self._tele_ptr)
            self._tele_seen[self._tele_ptr] = now
            self._tele_event = None
            slow = ((now[0] - seen[0]) & 0xFFFFFFFF) if seen is not None else 0
            if seen is not None and ((now[1] - seen[1]) & 0xFFFFFFFF) != 0:
                raise RuntimeError("sx_macenko_transform: a bounded wait inside the fused launch ran out on an earlier call (the device did not run its "
                                   "workgroups to completion); that call's output is incomplete")
            if slow > 0:
                self._classic_left = self._classic_span
                self._classic_span = min(self._classic_span * 2, 4096)      # probe again, less and less often
            else:
                self._classic_span = 32
                self._classic_left = 0      # (a probe that came back clean ends the provisional four-pass calls behind it)
        if self._classic_left > 0:
            self._classic_left -= 1
            return _native.MACENKO_CLASSIC
        if self._classic_span > 32 and self._tele_event is None:
            # A PROBE: the data was hard not long ago, and this call tries the two-pass form again.  Only this one: the calls behind it
            # stay with the four passes until its answer is in (a probe used to be every call up to the answer -- up to five calls at
            # 0.7 ms on real tissue, 10-20 us per step averaged over a loop of 200).
            self._classic_left = 8
        return 0

    def _watch(self, ws: torch.Tensor) -> None:
        """Read the library's counts of slow selections (and of waits that ran out) back without making anything wait: a side stream
        copies eight bytes once the call's kernels are done.  (Not inside a stream capture; advisory only.)"""
        if self._tele_event is not None or torch.cuda.is_current_stream_capturing():
            return
        if self._tele_host is None:
            self._tele_host = torch.zeros(2, dtype=torch.int32).pin_memory()
            self._tele_stream = torch.cuda.Stream(self.device)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        self._tele_stream.wait_event(done)
        with torch.cuda.stream(self._tele_stream):
            self._tele_host.copy_(ws[self._tele_offset:self._tele_offset + 8].view(torch.int32), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._tele_stream)
        ws.record_stream(self._tele_stream)
        self._tele_event = ev
        self._tele_ptr = ws.data_ptr()
        self._tele_age = 0

    def compute_reference_stain_matrix(self, images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Pooled stain estimate ``(HE (3,2), maxC (2,))`` (compute_reference_stain_matrix_torch, :463-519)."""
        images, n, h, w, code = self._images(images, False, "Macenko fit")
        he = torch.empty((3, 2), dtype=torch.float32, device=self.device)
        max_c = torch.empty((2,), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            ws = self._classic_workspace(code, n, h, w)
            self._call("sx_macenko_fit", images, code, n, h, w, he, max_c, ws, ws.numel())
        self.last_workspace = ws
        return he, max_c

    # name kept so code written against the reference's torch class keeps working
    compute_reference_stain_matrix_torch = compute_reference_stain_matrix

    # ---- staged pooled fit for a batch sharded across ranks (see stainx_amd/distributed.py) ----------
    # (the pooled fit's host path, profiled call by call -- tools/host_time_pooled.py: the dfit_* / pfit_* calls stay written out)
    def dfit_moments(self, images: torch.Tensor) -> torch.Tensor:
        images = images.to(self.device)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"Macenko fit expects NCHW with C=3, got shape {tuple(images.shape)}")
        images = images.contiguous()
        n, _, h, w = images.shape
        mom = torch.empty(20, dtype=torch.float64, device=self.device)
        with _native.on_device(self.device):
            ws = self._scratch.get(self._lib.sx_macenko_workspace_bytes_for(_dtype_code(images), n, h, w, _native.MACENKO_CLASSIC), self.device)
            rc = self._lib.sx_macenko_dfit_moments(images.data_ptr(), _dtype_code(images), n, h, w, mom.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_dfit_moments")
        return mom

    def dfit_begin(self, moments: torch.Tensor) -> torch.Tensor:
        state = torch.zeros(self._lib.sx_macenko_dfit_state_bytes(), dtype=torch.uint8, device=self.device)
        moments = moments.to(self.device, torch.float64).contiguous()
        with _native.on_device(self.device):
            rc = self._lib.sx_macenko_dfit_begin(moments.data_ptr(), state.data_ptr(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_dfit_begin")
        return state

    def dfit_histogram(self, images: torch.Tensor, state: torch.Tensor, stage: int) -> torch.Tensor:
        images = images.to(self.device).contiguous()
        n, _, h, w = images.shape
        hist = torch.empty((2, 256), dtype=torch.int64, device=self.device)
        with _native.on_device(self.device):
            rc = self._lib.sx_macenko_dfit_histogram(images.data_ptr(), _dtype_code(images), n, h, w, state.data_ptr(), int(stage), hist.data_ptr(),
                                                     _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_dfit_histogram")
        return hist

    def dfit_advance(self, state: torch.Tensor, stage: int, hist: torch.Tensor) -> None:
        hist = hist.to(self.device, torch.int64).contiguous()
        with _native.on_device(self.device):
            rc = self._lib.sx_macenko_dfit_advance(state.data_ptr(), int(stage), hist.data_ptr(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_dfit_advance")

    def dfit_result(self, state: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        he = torch.empty((3, 2), dtype=torch.float32, device=self.device)
        max_c = torch.empty((2,), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            rc = self._lib.sx_macenko_dfit_result(state.data_ptr(), he.data_ptr(), max_c.data_ptr(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_dfit_result")
        return he, max_c

    # ---- the same pooled fit across ranks on the bracket machinery (three passes; see stainx_amd/distributed.py) ----
    def _pfit_ws(self, n: int, h: int, w: int) -> torch.Tensor:
        need = self._pfit_bytes.get((n, h, w))
        if need is None:
            need = self._pfit_bytes[(n, h, w)] = int(self._lib.sx_macenko_workspace_bytes_for(_native.DTYPE_CODES[torch.float32], n, h, w, _native.MACENKO_CLASSIC))
        return self._scratch.get(need, self.device)

    def pfit_sample_count(self, n: int, h: int, w: int) -> int:
        return int(self._lib.sx_macenko_pfit_sample_count(n, h, w))

    def pfit_stats(self, images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Local raw moments (10 float64) and the local sample's optical density (3, 4096) float32."""
        images = images.to(self.device)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"Macenko fit expects NCHW with C=3, got shape {tuple(images.shape)}")
        images = images.contiguous()
        n, _, h, w = images.shape
        mom = torch.empty(10, dtype=torch.float64, device=self.device)
        sample = torch.empty((3, 4096), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_stats(images.data_ptr(), _dtype_code(images), n, h, w, mom.data_ptr(), sample.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_stats")
        self.last_workspace = ws
        return mom, sample

    def pfit_plane(self, moments: torch.Tensor, n_all: int, sample_union: torch.Tensor, sample_count: int, shape: tuple[int, int, int]) -> None:
        n, h, w = shape
        moments = moments.to(self.device, torch.float64).contiguous()
        sample_union = sample_union.to(self.device, torch.float32).contiguous()
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_plane(moments.data_ptr(), int(n_all), sample_union.data_ptr(), int(sample_count), n, h, w, ws.data_ptr(), ws.numel(),
                                                 _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_plane")

    def pfit_pass(self, images: torch.Tensor, stage: int, n_all: int, sample_count: int) -> torch.Tensor:
        images = images.to(self.device).contiguous()
        n, _, h, w = images.shape
        sums = torch.empty(_native.PFIT_SUMS, dtype=torch.int64, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_pass(images.data_ptr(), _dtype_code(images), n, h, w, int(stage), int(n_all), int(sample_count), sums.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_pass")
        return sums

    def pfit_gather(self, sums_global: torch.Tensor, stage: int, n_all: int, sample_count: int, shape: tuple[int, int, int], share: int) -> tuple[torch.Tensor, torch.Tensor]:
        n, h, w = shape
        sums_global = sums_global.to(self.device, torch.int64).contiguous()
        compact = torch.empty((2, int(share)), dtype=torch.int32, device=self.device)      # (only the first `counts` entries of a row are written and read: no fill)
        counts = torch.empty(2, dtype=torch.int32, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_gather(sums_global.data_ptr(), int(stage), int(n_all), int(sample_count), n, h, w, int(share), compact.data_ptr(), counts.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_gather")
        return compact, counts

    def pfit_finish(self, gathered_compact: torch.Tensor, gathered_counts: torch.Tensor, stage: int, n_all: int, sample_count: int, shape: tuple[int, int, int]):
        """Stage 0: nothing returned.  Stage 1: (HE, maxC, status) -- status is a device int32, non-zero if a bracket missed."""
        n, h, w = shape
        world, share = int(gathered_counts.shape[0]), int(gathered_compact.shape[-1])
        gathered_compact = gathered_compact.to(self.device, torch.int32).contiguous()
        gathered_counts = gathered_counts.to(self.device, torch.int32).contiguous()
        he = torch.empty((3, 2), dtype=torch.float32, device=self.device)
        max_c = torch.empty((2,), dtype=torch.float32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_finish(gathered_compact.data_ptr(), gathered_counts.data_ptr(), world, share, int(stage), int(n_all), int(sample_count), n, h, w,
                                                  he.data_ptr(), max_c.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_finish")
        self.last_workspace = ws
        return (he, max_c, status) if stage == 1 else None

    # ---- the same steps with the records of the exchanges packed and unpacked by the library (include/stainx_hip.h) ----
    def pfit_stats_packed(self, images: torch.Tensor) -> torch.Tensor:
        """This rank's stats record [int64 tiles | 10 fp64 moments | 3 x 4096 fp32 sample] as bytes, ready for the all-gather."""
        images = images.to(self.device)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"Macenko fit expects NCHW with C=3, got shape {tuple(images.shape)}")
        images = images.contiguous()
        n, _, h, w = images.shape
        record = torch.empty(_native.PFIT_STATS_RECORD_BYTES, dtype=torch.uint8, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_stats_packed(images.data_ptr(), _dtype_code(images), n, h, w, record.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_stats_packed")
        self.last_workspace = ws
        return record

    def pfit_empty_record(self) -> torch.Tensor:
        """The record of a rank without tiles (it still takes part in the exchange that tells every rank so)."""
        return torch.zeros(_native.PFIT_STATS_RECORD_BYTES, dtype=torch.uint8, device=self.device)

    def pfit_plane_packed(self, gathered: torch.Tensor, sample_counts: list[int], expected_tiles: torch.Tensor | None, n_all: int, sample_count: int,
                          shape: tuple[int, int, int]) -> torch.Tensor:
        """Every rank's stats record (world, record bytes) -> plane and angle brackets; returns the one-element int32 "some rank's
        tile count is not the expected one" flag (zero without `expected_tiles`)."""
        n, h, w = shape
        world = int(gathered.shape[0])
        gathered = gathered.contiguous()
        counts = (_c.c_int * world)(*[int(v) for v in sample_counts])
        stale = torch.empty(1, dtype=torch.int32, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_plane_packed(gathered.data_ptr(), world, _c.cast(counts, _c.c_void_p), expected_tiles.data_ptr() if expected_tiles is not None else None,
                                                        stale.data_ptr(), int(n_all), int(sample_count), n, h, w, ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_plane_packed")
        return stale

    def pfit_gather_packed(self, sums_global: torch.Tensor, stage: int, n_all: int, sample_count: int, shape: tuple[int, int, int], share: int, stale: torch.Tensor | None) -> torch.Tensor:
        n, h, w = shape
        sums_global = sums_global.to(self.device, torch.int64).contiguous()
        row = torch.empty(3 + 2 * int(share), dtype=torch.int32, device=self.device)      # (only the counted entries are written and read: no fill)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_gather_packed(sums_global.data_ptr(), int(stage), int(n_all), int(sample_count), n, h, w, int(share),
                                                         stale.data_ptr() if stale is not None else None, row.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_gather_packed")
        return row

    def pfit_finish_packed(self, gathered_rows: torch.Tensor, stage: int, n_all: int, sample_count: int, shape: tuple[int, int, int], share: int):
        """Stage 0: nothing returned.  Stage 1: (HE, maxC, status) -- bits 0-3 of the device int32: a bracket missed; bit 4: a stale flag."""
        n, h, w = shape
        world = int(gathered_rows.shape[0])
        gathered_rows = gathered_rows.contiguous()
        he = torch.empty((3, 2), dtype=torch.float32, device=self.device)
        max_c = torch.empty((2,), dtype=torch.float32, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        with _native.on_device(self.device):
            ws = self._pfit_ws(n, h, w)
            rc = self._lib.sx_macenko_pfit_finish_packed(gathered_rows.data_ptr(), world, int(share), int(stage), int(n_all), int(sample_count), n, h, w, he.data_ptr(), max_c.data_ptr(),
                                                         status.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr(self.device))
        self._check(rc, "sx_macenko_pfit_finish_packed")
        self.last_workspace = ws
        return (he, max_c, status) if stage == 1 else None

    def tile_params(self, n_groups: int) -> dict[str, torch.Tensor]:
        """Intermediates of the last transform (per tile) or fit (one pooled group); used by tests."""
        if self.last_workspace is None:
            raise RuntimeError("no transform / fit has run on this backend yet")
        raw = torch.empty((n_groups, _native.MACENKO_PARAM_FLOATS), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            self._call("sx_macenko_tile_params", self.last_workspace, n_groups, raw)
        raw = raw.cpu()
        return {"n_kept": raw[:, 0].long(), "use_all": raw[:, 1].long(), "vecs": raw[:, 2:8].reshape(-1, 3, 2), "phi_lo": raw[:, 8],
                "phi_hi": raw[:, 9], "he": raw[:, 10:16].reshape(-1, 3, 2), "max_c": raw[:, 16:18], "fell_back": raw[:, 18].long(),
                "n_candidates": raw[:, 19:23].long(), "cov": raw[:, 23:32].reshape(-1, 3, 3), "stamps_us": raw[:, 32:48]}


class VahadaneHIP(MacenkoHIP):
    """Vahadane's estimate (sparse NMF of the optical density with two atoms; include/stainx_hip.h: sx_vahadane_estimate) and the
    percentile concentrations of a given basis (sx_stain_max_concentrations).  Everything downstream of an estimate -- ``apply*``,
    ``separate_apply*`` -- is the Macenko engine's."""

    def _matrices(self, matrices: torch.Tensor, rows: int, name: str) -> torch.Tensor:
        matrices = self._f32(matrices).reshape(-1, 3, 2)
        if matrices.shape[0] not in (1, rows):
            raise ValueError(f"{name} must hold 1 or {rows} stain matrices, got {matrices.shape[0]}")
        return matrices

    def vahadane_estimate(self, images: torch.Tensor, init: torch.Tensor, *, regularizer: float = 0.1, iterations: int = 30, pooled: bool = False, masked: bool = False,
                          mask: torch.Tensor | None = None, luminosity_threshold: float = 0.8, max_conc: bool = True) -> dict[str, torch.Tensor | None]:
        """``he`` (rows, 3, 2), ``max_c`` (rows, 2) or None, ``pixels`` (rows,) int64 -- the exact |S| --; rows = N, or 1 with ``pooled``.
        ``init``: (1, 3, 2) or (rows, 3, 2).  ``masked``: over ``mask`` (N, H, W), or with ``mask=None`` over the luminosity rule's
        mask (an ``sx_tissue_mask`` launch in front).  A group without a masked-in pixel has NaN rows and 0 pixels."""
        images, n, h, w, code = self._images(images, False, "Macenko", "estimate")
        rows = 1 if pooled else n
        init = self._matrices(init, rows, "init")
        out = {
            "he": torch.empty((rows, 3, 2), dtype=torch.float32, device=self.device),
            "max_c": torch.empty((rows, 2), dtype=torch.float32, device=self.device) if max_conc else None,
            "pixels": torch.empty((rows,), dtype=torch.int64, device=self.device),
        }
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = self._mask_for(images, mask, luminosity_threshold) if masked else None
            ws = self._scratch.get(self._lib.sx_vahadane_workspace_bytes(code, n, h, w), self.device)
            self._call("sx_vahadane_estimate", images, code, n, h, w, mask, int(pooled), init, init.shape[0], float(regularizer), int(iterations), out["he"], out["max_c"],
                       out["pixels"], 0, ws, ws.numel())
        return out

    def max_concentrations(self, images: torch.Tensor, stain_matrices: torch.Tensor, *, pooled: bool = False, masked: bool = False, mask: torch.Tensor | None = None,
                           luminosity_threshold: float = 0.8) -> dict[str, torch.Tensor]:
        """The nearest-rank 99th percentiles of the concentrations of GIVEN bases (1 or rows) over each group's masked-in pixels:
        ``max_c`` (rows, 2) float32 and ``pixels`` (rows,) int64."""
        images, n, h, w, code = self._images(images, False, "Macenko", "max_concentrations")
        rows = 1 if pooled else n
        he = self._matrices(stain_matrices, rows, "stain_matrices")
        out = {"max_c": torch.empty((rows, 2), dtype=torch.float32, device=self.device), "pixels": torch.empty((rows,), dtype=torch.int64, device=self.device)}
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            mask = self._mask_for(images, mask, luminosity_threshold) if masked else None
            ws = self._scratch.get(self._lib.sx_vahadane_workspace_bytes(code, n, h, w), self.device)
            self._call("sx_stain_max_concentrations", images, code, n, h, w, mask, int(pooled), he, he.shape[0], out["max_c"], out["pixels"], 0, ws, ws.numel())
        return out


class LuminosityHIP(TorchHIPBackendBase):
    """Luminosity standardisation (include/stainx_hip.h: sx_luminosity_percentile, sx_luminosity_apply): the exact nearest-rank percentile
    of the luminance per tile or over the batch, and the one-launch map that makes it white.  Nothing synchronises; the percentile stays
    on the device and the apply pass reads it there."""

    def percentile(self, images: torch.Tensor, percentile: float, *, pooled: bool = False, mask: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(luminance, pixels)``: (rows,) float32 -- NaN for an empty set -- and (rows,) int64, rows = N or 1 with ``pooled``.  ``mask``:
        (N, H, W) uint8 / bool, which pixels enter the set."""
        images, n, h, w, code = self._images(images, False, None)
        rows = 1 if pooled else n
        luminance = torch.full((rows,), float("nan"), dtype=torch.float32, device=self.device)
        pixels = torch.zeros((rows,), dtype=torch.int64, device=self.device)
        if n * h * w == 0:
            return luminance, pixels
        mask = _mask_bytes(mask, self.device)
        with _native.on_device(self.device):
            ws = self._scratch.get(self._lib.sx_luminosity_workspace_bytes(code, n, h, w), self.device)
            self._call("sx_luminosity_percentile", images, code, n, h, w, mask, int(pooled), float(percentile), luminance, pixels, ws, ws.numel())
        return luminance, pixels

    def apply(self, images: torch.Tensor, luminance: torch.Tensor) -> torch.Tensor:
        """The map with GIVEN percentiles: ``luminance`` holds one row, or one per tile."""
        images, n, h, w, code = self._images(images, False, None)
        luminance = self._f32(luminance).reshape(-1)
        if luminance.shape[0] not in (1, n):
            raise ValueError(f"luminance must hold 1 or {n} rows, got {luminance.shape[0]}")
        out = torch.empty_like(images)
        if n * h * w != 0:
            with _native.on_device(self.device):
                self._call("sx_luminosity_apply", images, out, code, n, h, w, luminance, luminance.shape[0])
        return out


class DeconvHIP(TorchHIPBackendBase):
    """Three-stain colour deconvolution with a GIVEN (3, 3) basis (include/stainx_hip.h: sx_deconv_*): one kernel launch per call, no
    estimate, no workspace, no host synchronisation.  Bases, factors and masks are read on the device: a captured call replayed after
    new values are copied into the same tensors uses the new values."""

    def _bases(self, basis: torch.Tensor, n: int, what: str) -> tuple[torch.Tensor, int]:
        rows = _basis_rows(basis, n, what)
        return self._f32(basis), rows

    def apply(self, images: torch.Tensor, basis: torch.Tensor, target: torch.Tensor | None = None, *, alpha: torch.Tensor | None = None,
              beta: torch.Tensor | None = None, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False,
              masking: tuple | None = None) -> torch.Tensor:
        """``C' = alpha * inverse(basis) OD + beta`` rebuilt with ``target`` (None: ``basis``).  ``basis`` / ``target``: (3, 3), (1, 3, 3)
        or (N, 3, 3); ``alpha`` / ``beta``: (N, 3), both or neither.  ``masking``: None, or ``(explicit mask or None, luminosity
        threshold)`` -- the masked call (planar tiles only); the rule's mask is an ``sx_tissue_mask`` launch in front."""
        if masking is not None and channels_last:
            raise ValueError("a masked deconvolution takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "deconvolution", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        b, n_bases = self._bases(basis, n, "basis")
        t, n_targets = (None, 0) if target is None else self._bases(target, n, "target")
        if (alpha is None) != (beta is None):
            raise ValueError("alpha and beta go together: both or neither")
        fa = fb = None
        if alpha is not None:
            _check_factors(alpha, beta, n, 3)
            fa, fb = self._f32(alpha), self._f32(beta)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_deconv_apply", images, out, code, n, h, w, b, n_bases, t, n_targets, fa, fb, flags)
            else:
                self._call("sx_deconv_apply_masked", images, out, code, n, h, w, b, n_bases, t, n_targets, fa, fb, self._mask_for(images, *masking), flags)
        return out

    def separate(self, images: torch.Tensor, basis: torch.Tensor, *, stains: bool = True, concentrations: bool = False, normalize_to_0_1: bool = False,
                 out_dtype: torch.dtype | None = None, channels_last: bool = False) -> tuple[torch.Tensor | None, torch.Tensor | None]:
        """``(images (3, N, ...) or None, concentrations (N, 3, H, W) / (N, H, W, 3) float32 or None)``: image i is the tile rebuilt from
        stain i alone -- the bits of ``apply`` with ``alpha = e_i``."""
        if not stains and not concentrations:
            raise ValueError("separate: ask for the stain images, the concentrations, or both")
        images, n, h, w, code = self._images(images, channels_last, "deconvolution", "separate")
        flags, out_dtype = _out_flags(images, out_dtype if stains else None, normalize_to_0_1 and stains, channels_last)
        b, n_bases = self._bases(basis, n, "basis")
        imgs = torch.empty((3,) + tuple(images.shape), dtype=out_dtype, device=self.device) if stains else None
        conc = torch.empty((n, h, w, 3) if channels_last else (n, 3, h, w), dtype=torch.float32, device=self.device) if concentrations else None
        if n * h * w != 0:
            with _native.on_device(self.device):
                self._call("sx_deconv_separate", images, imgs, conc, code, n, h, w, b, n_bases, flags)
        return imgs, conc

    def combine(self, concentrations: torch.Tensor, basis: torch.Tensor, *, out_dtype: torch.dtype = torch.uint8, normalize_to_0_1: bool = False,
                channels_last: bool = False) -> torch.Tensor:
        """``separate``'s inverse: (N, 3, H, W) float32 concentrations (NHWC with ``channels_last``) -> the tile, cast to ``out_dtype``."""
        n, h, w = _image_shape(concentrations, channels_last, "deconvolution", "combine")
        if concentrations.dtype != torch.float32:
            raise ValueError(f"concentrations must be float32, got {concentrations.dtype}")
        if out_dtype not in _native.DTYPE_CODES:
            raise TypeError(f"unsupported out_dtype {out_dtype}; supported: {sorted(str(d) for d in _native.DTYPE_CODES)}")
        if normalize_to_0_1 and out_dtype == torch.uint8:
            raise ValueError("normalize_to_0_1 needs a float out_dtype (uint8 output stays on 0-255)")
        b, n_bases = self._bases(basis, n, "basis")
        conc = concentrations.to(self.device).contiguous()
        out = torch.empty(tuple(conc.shape), dtype=out_dtype, device=self.device)
        if n * h * w != 0:
            flags = (_native.MACENKO_NORMALIZE_0_1 if normalize_to_0_1 else 0) | (_native.MACENKO_CHANNELS_LAST if channels_last else 0)
            with _native.on_device(self.device):
                self._call("sx_deconv_combine", conc, out, _native.DTYPE_CODES[out_dtype], n, h, w, b, n_bases, flags)
        return out

    def _sums(self, what: str, images: torch.Tensor, basis: torch.Tensor, scalars: tuple, words: int, per_tile: bool, channels_last: bool, masking: tuple | None) -> torch.Tensor:
        """quantify / moments: the (S, words) int64 rows of ``sx_deconv_<what>[_masked]``, S = N (``per_tile``) or 1; zeros for an empty batch."""
        if masking is not None and channels_last:
            raise ValueError("a masked deconvolution takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "deconvolution", what)
        b, n_bases = self._bases(basis, n, "basis")
        sets = n if per_tile else 1
        if n * h * w == 0:
            return torch.zeros((sets, words), dtype=torch.int64, device=self.device)
        out = torch.empty((sets, words), dtype=torch.int64, device=self.device)
        flags = _native.MACENKO_CHANNELS_LAST if channels_last else 0
        with _native.on_device(self.device):
            if masking is None:
                self._call(f"sx_deconv_{what}", images, code, n, h, w, b, n_bases, *scalars, int(bool(per_tile)), out, flags)
            else:
                self._call(f"sx_deconv_{what}_masked", images, code, n, h, w, b, n_bases, *scalars, int(bool(per_tile)), out, self._mask_for(images, *masking), flags)
        return out

    QUANT_WORDS = 3 * 256 + 3 + 1      # a row of sx_deconv_quantify's output: [counts 3 x 256][sums 3][pixels 1]

    def quantify(self, images: torch.Tensor, basis: torch.Tensor, *, bin_log2: int = 5, zero_bin: int = 64, per_tile: bool = True, channels_last: bool = False,
                 masking: tuple | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(counts (S, 3, 256), sums (S, 3), pixels (S,))``, int64 views of ONE (S, 772) tensor; S = N (``per_tile``) or 1.  The
        histograms of the three concentrations ``separate`` would write, their fixed-point (2^-16) sums and the counted pixels: a memset
        and one launch, no map.  ``masking`` as in ``apply``."""
        if not (isinstance(bin_log2, int) and 0 <= bin_log2 <= 8):
            raise ValueError(f"bin_log2 must be an integer in [0, 8], got {bin_log2!r}")
        if not (isinstance(zero_bin, int) and 0 <= zero_bin <= 255):
            raise ValueError(f"zero_bin must be an integer in [0, 255], got {zero_bin!r}")
        out = self._sums("quantify", images, basis, (bin_log2, zero_bin), self.QUANT_WORDS, per_tile, channels_last, masking)
        return out[:, :768].view(out.shape[0], 3, 256), out[:, 768:771], out[:, 771]

    MOMENT_WORDS = 7      # a row of sx_deconv_moments' output: [sums 3][squares 3][pixels 1]

    def moments(self, images: torch.Tensor, basis: torch.Tensor, *, per_tile: bool = True, channels_last: bool = False,
                masking: tuple | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(sums (S, 3), squares (S, 3), pixels (S,))``, int64 views of ONE (S, 7) tensor; S = N (``per_tile``) or 1.  Fixed-point sums
        (2^-16) and sums of squares (2^-24) of the three concentrations ``separate`` would write, and the counted pixels: a memset and one
        launch, no map.  ``masking`` as in ``apply``."""
        out = self._sums("moments", images, basis, (), self.MOMENT_WORDS, per_tile, channels_last, masking)
        return out[:, 0:3], out[:, 3:6], out[:, 6]


class HsvHIP(TorchHIPBackendBase):
    """HSV colour jitter (include/stainx_hip.h: sx_hsv_apply): one kernel launch per call, no estimate, no workspace, no host
    synchronisation.  Rows and masks are read on the device: a captured call replayed after new rows are copied into the same tensor
    uses the new rows."""

    def apply(self, images: torch.Tensor, rows: torch.Tensor, *, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False,
              masking: tuple | None = None) -> torch.Tensor:
        """``rows``: (5,), (1, 5) or (N, 5) floats ``(dh, a_s, b_s, a_v, b_v)``; a row with a non-finite member leaves its tile as it
        is.  ``masking``: None, or ``(explicit mask or None, luminosity threshold)`` -- the masked call (planar tiles only); the rule's
        mask is an ``sx_tissue_mask`` launch in front."""
        if masking is not None and channels_last:
            raise ValueError("a masked HSV jitter takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "HSV", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _hsv_rows(rows, n)
        r = self._f32(rows)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_hsv_apply", images, out, code, n, h, w, r, n_rows, flags)
            else:
                self._call("sx_hsv_apply_masked", images, out, code, n, h, w, r, n_rows, self._mask_for(images, *masking), flags)
        return out


def _tone_rows(rows: torch.Tensor, n: int) -> int:
    """Rows of a tone jitter, (4,), (1, 4) or (N, 4): the number of rows, 1 or N."""
    shape = tuple(getattr(rows, "shape", ()))
    if isinstance(rows, torch.Tensor) and shape == (4,):
        return 1
    if isinstance(rows, torch.Tensor) and len(shape) == 2 and shape[1] == 4 and shape[0] in (1, n):
        return shape[0]
    raise ValueError(f"rows must be a tensor of shape (4,), (1, 4) or (N, 4) = ({n}, 4) holding (a, b, gamma, sigma), got {shape}")


def _tone_seeds(seeds: torch.Tensor | None, n: int) -> None:
    """Seeds of a tone jitter: None, or (N,) int64."""
    if seeds is None:
        return
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.int64 or tuple(seeds.shape) != (n,):
        raise ValueError(f"seeds must be None or an int64 tensor of shape (N,) = ({n},), got {getattr(seeds, 'dtype', type(seeds).__name__)} {tuple(getattr(seeds, 'shape', ()))}")


class ToneHIP(TorchHIPBackendBase):
    """Tone jitter and grey statistics (include/stainx_hip.h: sx_tone_apply, sx_grey_statistics): one kernel launch per call (a clearing
    memset or launch in front of the statistics), no workspace, no host synchronisation.  Rows, seeds and masks are read on the device: a
    captured call replayed after new values are copied into the same tensors uses the new values."""

    def apply(self, images: torch.Tensor, rows: torch.Tensor, seeds: torch.Tensor | None = None, *, shared_noise: bool = False, normalize_to_0_1: bool = False,
              out_dtype: torch.dtype | None = None, channels_last: bool = False, masking: tuple | None = None) -> torch.Tensor:
        """``rows``: (4,), (1, 4) or (N, 4) floats ``(a, b, gamma, sigma)``; a row with a non-finite member, ``gamma <= 0`` or
        ``sigma < 0`` leaves its tile as it is.  ``seeds``: None (no noise) or (N,) int64.  ``masking`` as ``HsvHIP.apply``."""
        if masking is not None and channels_last:
            raise ValueError("a masked tone jitter takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "tone jitter", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _tone_rows(rows, n)
        _tone_seeds(seeds, n)
        r = self._f32(rows)
        s = None if seeds is None else seeds.to(self.device).contiguous()
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_tone_apply", images, out, code, n, h, w, r, n_rows, s, int(bool(shared_noise)), flags)
            else:
                self._call("sx_tone_apply_masked", images, out, code, n, h, w, r, n_rows, s, int(bool(shared_noise)), self._mask_for(images, *masking), flags)
        return out

    def statistics(self, images: torch.Tensor, *, pooled: bool = False, channels_last: bool = False, masking: tuple | None = None) -> torch.Tensor:
        """(S, 3) int64 ``[pixels, sum Y, sum Y^2]``, S = N or 1 with ``pooled``; zeros for an empty batch.  ``masking`` as in ``apply``."""
        if masking is not None and channels_last:
            raise ValueError("masked grey statistics take planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, None)
        sets = 1 if pooled else n
        if n * h * w == 0:
            return torch.zeros((sets, 3), dtype=torch.int64, device=self.device)
        out = torch.empty((sets, 3), dtype=torch.int64, device=self.device)      # (the library clears what it adds into)
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_grey_statistics", images, code, n, h, w, int(channels_last), int(bool(pooled)), out)
            else:
                self._call("sx_grey_statistics_masked", images, code, n, h, w, 0, int(bool(pooled)), self._mask_for(images, *masking), out)
        return out


class BlurHIP(TorchHIPBackendBase):
    """Gaussian blur with a sigma per tile (include/stainx_hip.h: sx_gaussian_blur): one kernel launch per call, both passes on chip, no
    workspace, no host synchronisation.  Sigmas and masks are read on the device: a captured call replayed after new sigmas are copied
    into the same tensor uses the new sigmas."""

    def apply(self, images: torch.Tensor, sigmas: torch.Tensor, *, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False,
              masking: tuple | None = None) -> torch.Tensor:
        """``sigmas``: (), (1,) or (N,) floats; a sigma that is NaN, infinite, ``<= 0`` or below 0.125 leaves its tile as it is, one above
        4 is 4.  ``masking``: None, or ``(explicit mask or None, luminosity threshold)`` -- the masked call (planar tiles only); the
        rule's mask is an ``sx_tissue_mask`` launch in front."""
        if masking is not None and channels_last:
            raise ValueError("a masked Gaussian blur takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "Gaussian blur", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _sigma_rows(sigmas, n)
        s = self._f32(sigmas)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_gaussian_blur", images, out, code, n, h, w, s, n_rows, flags)
            else:
                self._call("sx_gaussian_blur_masked", images, out, code, n, h, w, s, n_rows, self._mask_for(images, *masking), flags)
        return out


def _quality_rows(qualities: torch.Tensor, n: int) -> int:
    """Qualities of a JPEG round trip, (), (1,) or (N,): the number of rows, 1 or N."""
    shape = tuple(getattr(qualities, "shape", (-1, -1)))
    if isinstance(qualities, torch.Tensor) and (shape == () or (len(shape) == 1 and shape[0] in (1, n))):
        return 1 if shape == () else shape[0]
    raise ValueError(f"quality must be an int or a tensor of shape (), (1,) or (N,) = ({n},), got {shape}")


class JpegHIP(TorchHIPBackendBase):
    """JPEG compression round trip with a quality per tile (include/stainx_hip.h: sx_jpeg_roundtrip): one kernel launch per call, encode
    and decode fused on chip, no bitstream, no workspace, no host synchronisation.  Qualities and masks are read on the device: a
    captured call replayed after new qualities are copied into the same tensor uses the new qualities."""

    def apply(self, images: torch.Tensor, qualities: torch.Tensor, subsampling: int = 2, *, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None,
              channels_last: bool = False, masking: tuple | None = None) -> torch.Tensor:
        """``qualities``: (), (1,) or (N,) floats; a quality that is NaN, infinite or ``< 1`` leaves its tile as it is, one above 100 is
        100.  ``subsampling``: 0 (4:4:4) or 2 (4:2:0).  ``masking``: None, or ``(explicit mask or None, luminosity threshold)`` -- the
        masked call (planar tiles only); the rule's mask is an ``sx_tissue_mask`` launch in front."""
        if subsampling not in (0, 2) or isinstance(subsampling, bool):
            raise ValueError(f"subsampling must be 0 (4:4:4) or 2 (4:2:0), got {subsampling!r}")
        if masking is not None and channels_last:
            raise ValueError("a masked JPEG round trip takes planar (NCHW) tiles only")
        images, n, h, w, code = self._images(images, channels_last, "JPEG round trip", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _quality_rows(qualities, n)
        q = self._f32(qualities)
        out = torch.empty(tuple(images.shape), dtype=out_dtype, device=self.device)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_jpeg_roundtrip", images, out, code, n, h, w, q, n_rows, subsampling, flags)
            else:
                self._call("sx_jpeg_roundtrip_masked", images, out, code, n, h, w, q, n_rows, subsampling, self._mask_for(images, *masking), flags)
        return out


class WarpHIP(TorchHIPBackendBase):
    """Affine warp with a row per tile (include/stainx_hip.h: sx_affine_warp, sx_affine_warp_mask): one kernel launch per call, no
    workspace, no host synchronisation.  Rows are read on the device: a captured call replayed after new rows are copied into the same
    tensor uses the new rows."""

    def apply(self, images: torch.Tensor, rows: torch.Tensor, size: tuple[int, int] | None = None, *, interpolation: str = "bilinear", border: str = "mirror", fill: float = 0.0,
              normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False) -> torch.Tensor:
        """``rows``: (6,), (1, 6) or (N, 6) floats, output pixel -> source position; a row with a NaN or an infinity leaves its tile
        (copy, centre crop or centre pad).  ``size``: (OH, OW) of the result, default the input's."""
        images, n, h, w, code = self._images(images, channels_last, "affine warp", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _warp_rows(rows, n)
        oh, ow = (h, w) if size is None else size
        r = self._f32(rows)
        out = torch.empty((n, oh, ow, 3) if channels_last else (n, 3, oh, ow), dtype=out_dtype, device=self.device)
        if n * h * w == 0 or oh * ow == 0:
            return out
        with _native.on_device(self.device):
            self._call("sx_affine_warp", images, out, code, n, h, w, oh, ow, r, n_rows, _native.WARP_INTERPOLATIONS[interpolation], _native.WARP_BORDERS[border], float(fill), flags)
        return out

    def apply_mask(self, mask: torch.Tensor, rows: torch.Tensor, size: tuple[int, int] | None = None, *, border: str = "constant", fill: int = 0) -> torch.Tensor:
        """``mask``: dense uint8 (N, H, W) -> uint8 (N, OH, OW): nearest, bytes moved as bytes."""
        mask = _mask_bytes(mask, self.device)
        n, h, w = mask.shape
        n_rows = _warp_rows(rows, n)
        oh, ow = (h, w) if size is None else size
        r = self._f32(rows)
        out = torch.empty((n, oh, ow), dtype=torch.uint8, device=self.device)
        if n * h * w == 0 or oh * ow == 0:
            return out
        with _native.on_device(self.device):
            self._call("sx_affine_warp_mask", mask, out, n, h, w, oh, ow, r, n_rows, _native.WARP_BORDERS[border], int(fill))
        return out


class ElasticHIP(TorchHIPBackendBase):
    """Elastic deformation fused with the affine warp (include/stainx_hip.h: sx_elastic_warp, sx_elastic_warp_mask): a row and a control
    grid per tile, one kernel launch per call, no workspace, no host synchronisation.  Rows and grids are read on the device."""

    def apply(self, images: torch.Tensor, rows: torch.Tensor, grids: torch.Tensor, cell: int, size: tuple[int, int] | None = None, *, interpolation: str = "bilinear",
              border: str = "mirror", fill: float = 0.0, normalize_to_0_1: bool = False, out_dtype: torch.dtype | None = None, channels_last: bool = False) -> torch.Tensor:
        """``rows`` as ``WarpHIP.apply``; ``grids``: (2, GH, GW), (1, 2, GH, GW) or (N, 2, GH, GW) floats for ``size`` and ``cell``."""
        images, n, h, w, code = self._images(images, channels_last, "elastic warp", "apply")
        flags, out_dtype = _out_flags(images, out_dtype, normalize_to_0_1, channels_last)
        n_rows = _warp_rows(rows, n)
        oh, ow = (h, w) if size is None else size
        n_grids = _elastic_grids(grids, n, oh, ow, cell)
        r, g = self._f32(rows), self._f32(grids)
        out = torch.empty((n, oh, ow, 3) if channels_last else (n, 3, oh, ow), dtype=out_dtype, device=self.device)
        if n * h * w == 0 or oh * ow == 0:
            return out
        with _native.on_device(self.device):
            self._call("sx_elastic_warp", images, out, code, n, h, w, oh, ow, r, n_rows, g, n_grids, int(cell), _native.WARP_INTERPOLATIONS[interpolation],
                       _native.WARP_BORDERS[border], float(fill), flags)
        return out

    def apply_mask(self, mask: torch.Tensor, rows: torch.Tensor, grids: torch.Tensor, cell: int, size: tuple[int, int] | None = None, *, border: str = "constant",
                   fill: int = 0) -> torch.Tensor:
        """``mask``: dense uint8 (N, H, W) -> uint8 (N, OH, OW): nearest, bytes moved as bytes."""
        mask = _mask_bytes(mask, self.device)
        n, h, w = mask.shape
        n_rows = _warp_rows(rows, n)
        oh, ow = (h, w) if size is None else size
        n_grids = _elastic_grids(grids, n, oh, ow, cell)
        r, g = self._f32(rows), self._f32(grids)
        out = torch.empty((n, oh, ow), dtype=torch.uint8, device=self.device)
        if n * h * w == 0 or oh * ow == 0:
            return out
        with _native.on_device(self.device):
            self._call("sx_elastic_warp_mask", mask, out, n, h, w, oh, ow, r, n_rows, g, n_grids, int(cell), _native.WARP_BORDERS[border], int(fill))
        return out


class ReinhardHIP(TorchHIPBackendBase):
    """Reinhard LAB statistics matching on the GPU (numerics of ReinhardTorch, torch_backend.py:304-355)."""

    def __init__(self, device: str | torch.device | None = None):
        super().__init__(device)
        self.last_workspace: torch.Tensor | None = None
        self._ws_shape: dict[int, tuple[int, int, int]] = {}      # workspace pointer -> the (n, h, w) of the last call on it (see _workspace)
        # workspaces of their own: the pooled transform's "last shape" bookkeeping is not touched by the per-tile and the masked calls
        self._tile_scratch = _native.Scratch()
        self._masked_scratch = _native.Scratch()

    def _workspace(self, n: int, h: int, w: int, ready: bool = False, code: int | None = None) -> torch.Tensor:
        """The stream's workspace.  Its arrival counters lie where (n, h, w) puts them and are zero between calls OF THAT SHAPE: the
        transform uses the entry point that relies on it (include/stainx_hip.h: sx_reinhard_transform_ready) and has the workspace
        zero-filled first whenever the last call on it had another shape (or there was none)."""
        # (`code`: the transform's element type -- a float32 batch gets room for its tiles' 8-bit codes behind the workspace proper)
        base = int(self._lib.sx_reinhard_workspace_bytes(n, h, w))
        ws = self._scratch.get(base if code is None else int(self._lib.sx_reinhard_workspace_bytes_for(code, n, h, w)), self.device)
        key = (int(n), int(h), int(w))
        if ready and self._ws_shape.get(ws.data_ptr()) != key:      # (the workspace proper: the codes behind it need no clearing)
            self._call("sx_reinhard_workspace_init", ws, base)
        self._ws_shape[ws.data_ptr()] = key
        self.last_workspace = ws
        return ws

    def _forget_shape(self) -> None:
        self._ws_shape.pop(self.last_workspace.data_ptr(), None)      # (a failed call may have left counters behind)

    def workspace_status(self) -> int:
        """Bit 0: a transform found the workspace not in its ready state (synchronises; for tests and diagnosis)."""
        ws = self.last_workspace
        off = int(self._lib.sx_reinhard_workspace_status_offset())
        return 0 if ws is None else int(ws[off:off + 4].view(torch.int32).item())

    def compute_reference_mean_std(self, images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        images, n, h, w, code = self._images(images, False, "Reinhard")
        mean = torch.empty(3, dtype=torch.float32, device=self.device)
        std = torch.empty(3, dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_reinhard_fit", images, code, n, h, w, mean, std, ws, ws.numel())
        return mean, std

    compute_reference_mean_std_torch = compute_reference_mean_std

    def transform(self, images: torch.Tensor, reference_mean: torch.Tensor, reference_std: torch.Tensor) -> torch.Tensor:
        images, n, h, w, code = self._images(images, False, "Reinhard")
        _reference_statistics(reference_mean, reference_std)
        mean, std = self._f32(reference_mean).flatten(), self._f32(reference_std).flatten()
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w, ready=True, code=code)
            self._call("sx_reinhard_transform_ready", images, out, code, n, h, w, mean, std, ws, ws.numel(), on_failure=self._forget_shape)
        return out

    # ---- per-tile statistics, given statistics (include/stainx_hip.h: sx_reinhard_tile_stats ...) ---------
    def tile_statistics(self, images: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """LAB mean and unbiased standard deviation of every tile: two (N, 3) float32 tensors, one statistics pass."""
        images, n, h, w, code = self._images(images, False, "Reinhard")
        mean = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        std = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        if n * h * w != 0:
            with _native.on_device(self.device):
                ws = self._tile_scratch.get(int(self._lib.sx_reinhard_tiles_workspace_bytes(code, n, h, w)), self.device)
                self._call("sx_reinhard_tile_stats", images, code, n, h, w, mean, std, ws, ws.numel())
        return mean, std

    def transform_tiles(self, images: torch.Tensor, reference_mean: torch.Tensor, reference_std: torch.Tensor, *, return_statistics: bool = False):
        """Every tile normalised with its OWN statistics (two streaming launches for the batch).  With ``return_statistics`` also the
        tiles' (N, 3) mean and standard deviation."""
        images, n, h, w, code = self._images(images, False, "Reinhard")
        _reference_statistics(reference_mean, reference_std)
        mean, std = self._f32(reference_mean).flatten(), self._f32(reference_std).flatten()
        out = torch.empty_like(images)
        tile_mean = tile_std = None
        if return_statistics:
            tile_mean = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            tile_std = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        if n * h * w != 0:
            with _native.on_device(self.device):
                ws = self._tile_scratch.get(int(self._lib.sx_reinhard_tiles_workspace_bytes(code, n, h, w)), self.device)
                self._call("sx_reinhard_transform_tiles", images, out, code, n, h, w, mean, std, tile_mean, tile_std, ws, ws.numel())
        return (out, tile_mean, tile_std) if return_statistics else out

    def apply_statistics(self, images: torch.Tensor, source_mean: torch.Tensor, source_std: torch.Tensor, reference_mean: torch.Tensor, reference_std: torch.Tensor) -> torch.Tensor:
        """Normalise with GIVEN source statistics, (1, 3) for the whole batch or (N, 3) per tile: one launch, no workspace."""
        return self._apply_statistics(images, source_mean, source_std, reference_mean, reference_std, None)

    # ---- tissue masks (include/stainx_hip.h: sx_reinhard_stats_masked ...) --------------------------------
    def masked_statistics(self, images: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float, *, per_tile: bool):
        """LAB mean / unbiased standard deviation over TISSUE pixels -- ``mask`` (N, H, W) uint8, or None: the luminosity rule -- of every
        tile (``per_tile``: (N, 3) each) or pooled over the batch ((1, 3) each), and the tissue counts (int64).  Fewer than two tissue
        pixels: a row of NaN."""
        images, n, h, w, code = self._images(images, False, "Reinhard")
        rows = n if per_tile else 1
        mean = torch.empty((rows, 3), dtype=torch.float32, device=self.device)
        std = torch.empty((rows, 3), dtype=torch.float32, device=self.device)
        counts = torch.zeros((rows,), dtype=torch.int64, device=self.device)
        if n * h * w == 0:
            return mean.fill_(float("nan")), std.fill_(float("nan")), counts
        mask = _mask_bytes(mask, self.device)
        with _native.on_device(self.device):
            ws = self._masked_scratch.get(int(self._lib.sx_reinhard_masked_workspace_bytes(code, n, h, w)), self.device)
            self._call("sx_reinhard_stats_masked", images, code, n, h, w, mask, float(luminosity_threshold), int(per_tile), mean, std, counts, ws, ws.numel())
        return mean, std, counts

    def transform_masked(self, images: torch.Tensor, reference_mean: torch.Tensor, reference_std: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float, *,
                         per_tile: bool, return_statistics: bool = False):
        """Tissue pixels normalised with the statistics of the tissue (per tile, or pooled over the batch), background pixels copied: two
        streaming launches.  With ``return_statistics`` also mean, std and the tissue counts."""
        images, n, h, w, code = self._images(images, False, "Reinhard")
        _reference_statistics(reference_mean, reference_std)
        mean, std = self._f32(reference_mean).flatten(), self._f32(reference_std).flatten()
        rows = n if per_tile else 1
        out = torch.empty_like(images)
        src_mean = src_std = counts = None
        if return_statistics:
            src_mean = torch.empty((rows, 3), dtype=torch.float32, device=self.device)
            src_std = torch.empty((rows, 3), dtype=torch.float32, device=self.device)
            counts = torch.zeros((rows,), dtype=torch.int64, device=self.device)
        if n * h * w != 0:
            mask = _mask_bytes(mask, self.device)
            with _native.on_device(self.device):
                ws = self._masked_scratch.get(int(self._lib.sx_reinhard_masked_workspace_bytes(code, n, h, w)), self.device)
                self._call("sx_reinhard_transform_masked", images, out, code, n, h, w, mean, std, mask, float(luminosity_threshold), int(per_tile), src_mean, src_std, counts,
                           ws, ws.numel())
        return (out, src_mean, src_std, counts) if return_statistics else out

    def apply_statistics_masked(self, images: torch.Tensor, source_mean: torch.Tensor, source_std: torch.Tensor, reference_mean: torch.Tensor, reference_std: torch.Tensor,
                                mask: torch.Tensor | None, luminosity_threshold: float) -> torch.Tensor:
        """``apply_statistics`` with a tissue mask: one launch; background pixels, and tiles whose row of statistics holds a NaN, are copied."""
        return self._apply_statistics(images, source_mean, source_std, reference_mean, reference_std, (mask, luminosity_threshold))

    def _apply_statistics(self, images, source_mean, source_std, reference_mean, reference_std, masking):
        images, n, h, w, code = self._images(images, False, "Reinhard")
        src_mean, src_std = _statistics_rows(source_mean, source_std, n, "source", "(1, 3)")
        src_mean, src_std = self._f32(src_mean), self._f32(src_std)
        _reference_statistics(reference_mean, reference_std)
        mean, std = self._f32(reference_mean).flatten(), self._f32(reference_std).flatten()
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_reinhard_apply_stats", images, out, code, n, h, w, src_mean, src_std, int(src_mean.shape[0]), mean, std)
            else:
                self._call("sx_reinhard_apply_stats_masked", images, out, code, n, h, w, src_mean, src_std, int(src_mean.shape[0]), mean, std, _mask_bytes(masking[0], self.device),
                           float(masking[1]))
        return out

    # ---- a target per tile (include/stainx_hip.h: sx_reinhard_apply_targets ...) --------------------------
    def apply_targets(self, images: torch.Tensor, source_mean: torch.Tensor, source_std: torch.Tensor, target_mean: torch.Tensor, target_std: torch.Tensor) -> torch.Tensor:
        """``apply_statistics`` with a row of TARGET statistics per tile as well -- (1, 3) or (N, 3) each: one launch, no workspace.  A
        tile any of whose rows holds a NaN is copied bit for bit."""
        return self._apply_targets(images, source_mean, source_std, target_mean, target_std, None)

    def apply_targets_masked(self, images: torch.Tensor, source_mean: torch.Tensor, source_std: torch.Tensor, target_mean: torch.Tensor, target_std: torch.Tensor,
                             mask: torch.Tensor | None, luminosity_threshold: float) -> torch.Tensor:
        """``apply_targets`` with a tissue mask (None: the luminosity rule): one launch; background pixels are copied."""
        return self._apply_targets(images, source_mean, source_std, target_mean, target_std, (mask, luminosity_threshold))

    def _apply_targets(self, images, source_mean, source_std, target_mean, target_std, masking):
        images, n, h, w, code = self._images(images, False, "Reinhard")
        source_mean, source_std = _statistics_rows(source_mean, source_std, n, "source")
        target_mean, target_std = _statistics_rows(target_mean, target_std, n, "target")
        sm, ss, tm, ts = self._f32(source_mean), self._f32(source_std), self._f32(target_mean), self._f32(target_std)
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_reinhard_apply_targets", images, out, code, n, h, w, sm, ss, int(sm.shape[0]), tm, ts, int(tm.shape[0]))
            else:
                self._call("sx_reinhard_apply_targets_masked", images, out, code, n, h, w, sm, ss, int(sm.shape[0]), tm, ts, int(tm.shape[0]), _mask_bytes(masking[0], self.device),
                           float(masking[1]))
        return out

    # ---- batch statistics pooled across ranks (see stainx_amd/distributed.py) --------------------------
    def local_sums(self, images: torch.Tensor) -> torch.Tensor:
        """6 fp64 values: per channel sum and sum of squares of (LAB - 128) over this rank's pixels."""
        images, n, h, w, code = self._images(images, False, "Reinhard")
        sums = torch.empty(6, dtype=torch.float64, device=self.device)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_reinhard_sums", images, code, n, h, w, sums, ws, ws.numel())
        return sums

    def apply_with_sums(self, images: torch.Tensor, sums: torch.Tensor, n_total_pixels: int, reference_mean: torch.Tensor, reference_std: torch.Tensor) -> torch.Tensor:
        images, n, h, w, code = self._images(images, False, "Reinhard")
        mean, std = self._f32(reference_mean).flatten(), self._f32(reference_std).flatten()
        sums = sums.to(self.device, torch.float64).contiguous()
        out = torch.empty_like(images)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_reinhard_apply", images, out, code, n, h, w, sums, float(n_total_pixels), mean, std, ws, ws.numel())
        return out


class HistogramMatchingHIP(TorchHIPBackendBase):
    """Histogram matching on the GPU (numerics of HistogramMatchingTorch, torch_backend.py:134-301)."""

    _ref_cache: tuple | None = None      # (a class default: a test of the cache builds the object without its device checks)

    def __init__(self, device: str | torch.device | None = None, channel_axis: int = 1, diag: bool = False):
        super().__init__(device)
        if diag:      # tests / tools: the diagnostic build (the one-launch design study lives there)
            self._lib = _native.require_diag()
        self.channel_axis = channel_axis
        self.last_workspace: torch.Tensor | None = None
        # the workspace is zero-filled when it is made and every library call leaves it zeroed again: the sx_hm_*_ready entry
        # points, which have no clearing launch in front of the histogram pass (include/stainx_hip.h)
        self._scratch = _native.Scratch(zeroed=True)
        # workspaces of their own (their calls clear what they need): the zeroed scratch of the pooled calls is not touched
        self._tile_scratch = _native.Scratch()
        self._masked_scratch = _native.Scratch()
        self._status_offset = int(self._lib.sx_hm_workspace_status_offset())

    def _drop_workspace(self) -> None:
        self._scratch.drop(self.device)      # (a failed call may have left counters behind)

    def workspace_status(self) -> int:
        """Bit 0: a call found the workspace not in its ready state (synchronises; for tests and diagnosis)."""
        ws = self.last_workspace
        return 0 if ws is None else int(ws[self._status_offset:self._status_offset + 4].view(torch.int32).item())

    def _channels_last(self, images: torch.Tensor) -> bool:
        return self.channel_axis == -1 or (self.channel_axis == 3 and images.ndim == 4)      # torch_backend.py:182

    def _workspace(self, n: int, h: int, w: int) -> torch.Tensor:
        return self._scratch.get(self._lib.sx_hm_workspace_bytes(n, h, w), self.device)

    def _tiles_workspace(self, n: int, h: int, w: int) -> torch.Tensor:
        return self._tile_scratch.get(int(self._lib.sx_hm_tiles_workspace_bytes(n, h, w)), self.device)

    def _masked_workspace(self, n: int, h: int, w: int) -> torch.Tensor:
        return self._masked_scratch.get(int(self._lib.sx_hm_masked_workspace_bytes(n, h, w)), self.device)

    def compute_reference_histograms(self, images: torch.Tensor) -> list[torch.Tensor]:
        """Three normalised 256-bin histograms, what ``transform`` receives (torch_backend.py:139-160)."""
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        hists = torch.empty((3, 256), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_hm_fit_ready", images, code, n, h, w, last, hists, ws, ws.numel(), on_failure=self._drop_workspace)
        return [hists[c] for c in range(3)]

    def _stack_reference(self, reference_histogram, chans: int) -> torch.Tensor:
        # list -> (C,256): pad with the first histogram / trim (torch_cuda_backend.py:51-74).  The normaliser hands over the same
        # fitted tensors on every call: the stacked copy is kept while they are the same objects at the same version (the
        # torch.stack was a 5 us kernel and a launch gap in front of every transform).
        # Not cached: tensors made under torch.inference_mode() (they track no version: an in-place change would go unseen -- and
        # reading `_version` raises), and anything while a stream capture is on (the stacked copy would only be filled at replay).
        parts = tuple(reference_histogram) if isinstance(reference_histogram, (list, tuple)) else (reference_histogram,)
        cacheable = (all(isinstance(p, torch.Tensor) and not p.is_inference() for p in parts)
                     and not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()))
        if not cacheable:
            return self._stack_reference_uncached(reference_histogram, chans)
        stamp = tuple((p.data_ptr(), tuple(p.shape), p._version) for p in parts)
        cached = self._ref_cache
        if (cached is not None and cached[0] == chans and len(cached[1]) == len(parts)
                and all(p is q for p, q in zip(parts, cached[1])) and cached[2] == stamp):
            return cached[3]
        ref = self._stack_reference_uncached(reference_histogram, chans)
        self._ref_cache = (chans, parts, stamp, ref)      # (holds the sources: their identities cannot be reused meanwhile)
        return ref

    def _stack_reference_uncached(self, reference_histogram, chans: int) -> torch.Tensor:
        if isinstance(reference_histogram, (list, tuple)):
            if len(reference_histogram) == 0:
                raise ValueError("reference_histogram list cannot be empty")
            for i, hist in enumerate(reference_histogram):
                if not isinstance(hist, torch.Tensor):
                    raise TypeError(f"reference_histogram[{i}] must be a torch.Tensor, got {type(hist)}")
                if hist.dim() != 1 or hist.size(0) != 256:
                    raise ValueError(f"Each histogram in reference_histogram list must be 1D with 256 elements. Got histogram at index {i} with shape {hist.shape}")
            rows = [h.to(self.device) for h in reference_histogram]
            while len(rows) < chans:
                rows.append(rows[0])
            ref = torch.stack(rows[:chans], dim=0)
        else:
            ref = reference_histogram.to(self.device)
            if ref.dim() != 1 or ref.size(0) != 256:
                raise ValueError(f"reference_histogram must be 1D with 256 elements. Got shape {ref.shape}")
            ref = ref.unsqueeze(0).expand(chans, 256)
        return ref.to(torch.float32).contiguous()

    def transform(self, images: torch.Tensor, reference_histogram) -> torch.Tensor:
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        ref = self._stack_reference(reference_histogram, 3)
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_hm_transform_ready", images, out, code, n, h, w, last, ref, ws, ws.numel(), on_failure=self._drop_workspace)
        self.last_workspace = ws
        return out

    # ---- one histogram and one LUT per tile (include/stainx_hip.h: sx_hm_transform_tiles) ------------------
    def transform_tiles(self, images: torch.Tensor, reference_histogram) -> torch.Tensor:
        """Every tile matched to the reference with its OWN histogram: three launches for the batch, tile t's bits those of
        ``transform(images[t:t+1])``."""
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        ref = self._stack_reference(reference_histogram, 3)
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            ws = self._tiles_workspace(n, h, w)
            self._call("sx_hm_transform_tiles", images, out, code, n, h, w, last, ref, None, None, ws, ws.numel())
        self._last_tiles = (ws, int(n), int(self._lib.sx_hm_workspace_bytes(n, h, w)))
        return out

    def tile_tables(self) -> dict[str, torch.Tensor]:
        """Integer source histograms (N,3,256) and float LUTs (N,3,256) of the last per-tile transform."""
        ws, n, base = self._last_tiles
        words = n * 3 * 256
        counts = ws[base + 4 * words: base + 8 * words].view(torch.int32).reshape(n, 3, 256).cpu().long()
        lut = ws[base + 8 * words: base + 12 * words].view(torch.float32).reshape(n, 3, 256).cpu()
        return {"counts": counts, "lut": lut}

    # ---- tissue masks (include/stainx_hip.h: sx_hm_fit_masked, sx_hm_transform_masked) ----------------------
    def compute_reference_histograms_masked(self, images: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float) -> list[torch.Tensor]:
        """``compute_reference_histograms`` over TISSUE pixels only (``mask`` (N, H, W) uint8, or None: the luminosity rule)."""
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        hists = torch.empty((3, 256), dtype=torch.float32, device=self.device)
        count = torch.zeros((1,), dtype=torch.int64, device=self.device)
        mask = _mask_bytes(mask, self.device)
        with _native.on_device(self.device):
            ws = self._masked_workspace(n, h, w)
            self._call("sx_hm_fit_masked", images, code, n, h, w, last, mask, float(luminosity_threshold), hists, count, ws, ws.numel())
        self.last_workspace = ws
        self.last_tissue_count = count
        return [hists[c] for c in range(3)]

    def transform_masked(self, images: torch.Tensor, reference_histogram, mask: torch.Tensor | None, luminosity_threshold: float, *, per_tile: bool,
                         return_tables: bool = False):
        """Tissue pixels matched with the histogram(s) of the tissue -- one per tile, or one pooled over the batch --, background pixels
        copied with the bits of the input.  With ``return_tables`` also a dict: ``counts`` (sets, 3, 256) int32 histograms as counted,
        ``lut`` (sets, 3, 256) float LUTs, ``tissue`` (sets,) int64 tissue pixels (sets = N per tile, 1 pooled)."""
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        ref = self._stack_reference(reference_histogram, 3)
        out = torch.empty_like(images)
        sets = n if per_tile else 1
        tables = {"counts": None, "lut": None, "tissue": None}
        if return_tables:
            tables = {"counts": torch.zeros((sets, 3, 256), dtype=torch.int32, device=self.device), "lut": torch.zeros((sets, 3, 256), dtype=torch.float32, device=self.device),
                      "tissue": torch.zeros((sets,), dtype=torch.int64, device=self.device)}
        if n * h * w != 0:
            mask = _mask_bytes(mask, self.device)
            with _native.on_device(self.device):
                ws = self._masked_workspace(n, h, w)
                self._call("sx_hm_transform_masked", images, out, code, n, h, w, last, ref, mask, float(luminosity_threshold), int(per_tile), tables["counts"], tables["lut"],
                           tables["tissue"], ws, ws.numel())
            self.last_workspace = ws
        return (out, tables) if return_tables else out

    # ---- slide level: estimate histograms, tables from given counts, apply given tables (include/stainx_hip.h: sx_hm_estimate ...) ----
    def estimate_histograms(self, images: torch.Tensor, *, per_tile: bool, masked: bool = False, mask: torch.Tensor | None = None,
                            luminosity_threshold: float = 0.8) -> tuple[torch.Tensor, torch.Tensor]:
        """The histogram pass alone: ``counts`` (sets, 3, 256) int64 and ``pixels`` (sets,) int64 on the device, sets = N per tile or 1
        pooled over the batch.  ``masked``: tissue pixels only (``mask`` (N, H, W) uint8, or None: the luminosity rule)."""
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        sets = n if per_tile else 1
        counts = torch.zeros((sets, 3, 256), dtype=torch.int64, device=self.device)
        pixels = torch.zeros((sets,), dtype=torch.int64, device=self.device)
        if n * h * w == 0:
            return counts, pixels
        mask = _mask_bytes(mask, self.device) if masked else None
        with _native.on_device(self.device):
            if masked:
                ws = self._masked_workspace(n, h, w)
                self._call("sx_hm_estimate_masked", images, code, n, h, w, last, int(per_tile), mask, float(luminosity_threshold), counts, pixels, ws, ws.numel())
            else:
                ws = self._tiles_workspace(n, h, w)
                self._call("sx_hm_estimate", images, code, n, h, w, last, int(per_tile), counts, pixels, ws, ws.numel())
        self.last_workspace = ws
        return counts, pixels

    def lookup_tables(self, counts: torch.Tensor, pixels: torch.Tensor, reference_histogram) -> torch.Tensor:
        """(S, 3, 256) float32 lookup tables from GIVEN counts (S, 3, 256) and pixel totals (S,): one launch.  A set without pixels gets
        the identity table."""
        if counts.dim() != 3 or tuple(counts.shape[1:]) != (3, 256) or counts.shape[0] < 1:
            raise ValueError(f"counts must have shape (S, 3, 256) with S >= 1, got {tuple(counts.shape)}")
        if tuple(pixels.shape) != (counts.shape[0],):
            raise ValueError(f"pixels must have shape (S,) = ({counts.shape[0]},), got {tuple(pixels.shape)}")
        counts = counts.to(self.device, torch.int64).contiguous()
        pixels = pixels.to(self.device, torch.int64).contiguous()
        ref = self._stack_reference(reference_histogram, 3)
        lut = torch.empty(tuple(counts.shape), dtype=torch.float32, device=self.device)
        with _native.on_device(self.device):
            self._call("sx_hm_tables", counts, pixels, int(counts.shape[0]), ref, lut)
        return lut

    def _given_tables(self, tables: torch.Tensor, n: int) -> torch.Tensor:
        if tables.dim() == 2:
            tables = tables.unsqueeze(0)
        if tables.dim() != 3 or tuple(tables.shape[1:]) != (3, 256) or tables.shape[0] not in (1, n):
            raise ValueError(f"tables must be (3, 256), (1, 3, 256) or ({n}, 3, 256) for {n} tiles, got shape {tuple(tables.shape)}")
        if tables.dtype != torch.float32:
            raise ValueError(f"tables must be float32, got {tables.dtype}")
        return tables.to(self.device).contiguous()

    def apply_tables(self, images: torch.Tensor, tables: torch.Tensor) -> torch.Tensor:
        """Normalise with GIVEN float lookup tables, (1, 3, 256) for the whole batch or (N, 3, 256) per tile: one launch, no workspace."""
        return self._apply_tables(images, tables, None)

    def apply_tables_masked(self, images: torch.Tensor, tables: torch.Tensor, mask: torch.Tensor | None, luminosity_threshold: float) -> torch.Tensor:
        """``apply_tables`` with a tissue mask: one launch; background pixels are copied with the bits of the input."""
        return self._apply_tables(images, tables, (mask, luminosity_threshold))

    def _apply_tables(self, images, tables, masking):
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        tables = self._given_tables(tables, n)
        out = torch.empty_like(images)
        if n * h * w == 0:
            return out
        with _native.on_device(self.device):
            if masking is None:
                self._call("sx_hm_apply_tables", images, out, code, n, h, w, last, tables, int(tables.shape[0]))
            else:
                self._call("sx_hm_apply_tables_masked", images, out, code, n, h, w, last, tables, int(tables.shape[0]), _mask_bytes(masking[0], self.device), float(masking[1]))
        return out

    # ---- source histogram pooled across ranks (see stainx_amd/distributed.py) --------------------------
    def local_counts(self, images: torch.Tensor) -> torch.Tensor:
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        counts = torch.empty((3, 256), dtype=torch.int64, device=self.device)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_hm_counts_ready", images, code, n, h, w, last, counts, ws, ws.numel(), on_failure=self._drop_workspace)
        return counts

    def apply_with_counts(self, images: torch.Tensor, counts: torch.Tensor, n_total_pixels: int, reference_histogram) -> torch.Tensor:
        last = int(self._channels_last(images))
        images, n, h, w, code = self._images(images, last, "HistogramMatching")
        ref = self._stack_reference(reference_histogram, 3)
        counts = counts.to(self.device, torch.int64).contiguous()
        out = torch.empty_like(images)
        with _native.on_device(self.device):
            ws = self._workspace(n, h, w)
            self._call("sx_hm_apply", images, out, code, n, h, w, last, counts, float(n_total_pixels), ref, ws, ws.numel())
        self.last_workspace = ws
        return out

    def tables(self) -> dict[str, torch.Tensor]:
        """Pooled integer source histogram (3,256) and float LUT (3,256) of the last transform."""
        ws = self.last_workspace
        counts = ws[: 3 * 256 * 4].view(torch.int32).reshape(3, 256).cpu().long()
        lut = ws[3 * 256 * 4 : 2 * 3 * 256 * 4].view(torch.float32).reshape(3, 256).cpu()
        return {"counts": counts, "lut": lut}
