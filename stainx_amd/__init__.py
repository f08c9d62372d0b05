"""stainx_amd -- MI355X-native (gfx950) stain normalisation behind stainx's fit/transform API.

Drop-in surface: ``Macenko``, ``Reinhard``, ``HistogramMatching``, ``StainNormalizerTransform``,
``StainNormalizerBase`` (reference src/stainx/__init__.py); ``Vahadane`` (an extension: Macenko's surface with Vahadane's sparse-NMF stain estimate); ``MacenkoAugment`` (an extension: H&E stain augmentation); ``ColorDeconvolution``, ``HEDAugment``, ``stain_basis``, ``complement_basis`` (an extension: three-stain colour deconvolution with a given basis -- HED, H-DAB); ``StainSeparation`` (what ``Macenko.separate``, an extension, returns); ``StainEstimate`` (a source stain basis: ``Macenko.estimate`` returns it, ``Macenko.apply`` takes it); ``ColorStatistics`` (LAB statistics of a source: ``Reinhard.estimate`` returns it, ``Reinhard.apply`` takes it); ``HistogramStatistics`` (integer histograms of a source: ``HistogramMatching.estimate`` returns it, ``lookup_tables`` and ``apply`` take it); ``tissue_mask`` (the luminosity rule of the opt-in tissue masks of ``Reinhard`` and ``HistogramMatching``); ``luminosity_histogram``, ``otsu_threshold``, ``otsu_mask``, ``mask_morphology``, ``refine_mask`` (tissue detection: an Otsu threshold taken from the data and a morphological clean-up of the mask; ``LuminosityHistogram`` and ``TissueDetection`` are what they return); ``mask_components``, ``remove_small_objects``, ``remove_small_holes`` (connected components of masks and the filters by area; ``MaskComponents`` is what the first returns); ``saturation_map``, ``median_filter``, ``level_histogram``, ``otsu_level``, ``level_mask``, ``saturation_mask`` (tissue detection on the HSV saturation after a median filter, CLAM's rule; ``LevelHistogram`` and ``SaturationDetection`` are what they return); ``LuminosityStandardizer`` (brightness standardisation, staintools' first step: the exact L* percentile becomes white; ``LuminosityEstimate`` is what its ``estimate`` returns and its ``apply`` takes); ``sample_pixels`` (tissue pixel sampling: a fixed-shape tile of at most K masked-in pixels per tile or per batch, chosen by an exact integer rule and copied bit for bit -- what a slide-level estimate reads; ``PixelSample`` is what it returns, ``PixelSample.cat`` joins the samples of several batches).  Importing the package never touches
the GPU; the native library is loaded when a backend is first instantiated and its absence raises.
"""
from stainx_amd.augment import MacenkoAugment
from stainx_amd.base import StainNormalizerBase
from stainx_amd.deconv import ColorDeconvolution, DeconvSeparation, HEDAugment, StainHistograms, complement_basis, stain_basis
from stainx_amd.luminosity import LuminosityEstimate, LuminosityStandardizer
from stainx_amd.masks import (LevelHistogram, LuminosityHistogram, MaskComponents, SaturationDetection, TissueDetection, level_histogram, level_mask, luminosity_histogram,
                              mask_components, mask_morphology, median_filter, otsu_level, otsu_mask, otsu_threshold, refine_mask, remove_small_holes, remove_small_objects,
                              saturation_map, saturation_mask, tissue_mask)
from stainx_amd.normalizers import HistogramMatching, Macenko, Reinhard, Vahadane
from stainx_amd.normalizers.histogram_matching import HistogramStatistics
from stainx_amd.normalizers.macenko import StainEstimate, StainSeparation
from stainx_amd.normalizers.reinhard import ColorStatistics
from stainx_amd.sampling import PixelSample, sample_pixels
from stainx_amd.transforms import StainNormalizerTransform

__version__ = "0.1.0"
__all__ = ["ColorDeconvolution", "ColorStatistics", "DeconvSeparation", "HEDAugment", "HistogramMatching", "HistogramStatistics", "LevelHistogram", "LuminosityEstimate", "LuminosityHistogram", "LuminosityStandardizer", "Macenko", "MacenkoAugment", "MaskComponents", "PixelSample", "Reinhard", "SaturationDetection", "StainNormalizerBase", "StainEstimate", "StainHistograms", "StainNormalizerTransform", "StainSeparation", "TissueDetection", "Vahadane", "complement_basis", "level_histogram", "level_mask", "luminosity_histogram", "mask_components", "mask_morphology", "median_filter", "otsu_level", "otsu_mask", "otsu_threshold", "refine_mask", "remove_small_holes", "remove_small_objects", "sample_pixels", "saturation_map", "saturation_mask", "stain_basis", "tissue_mask", "__version__"]
