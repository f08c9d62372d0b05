from stainx_amd.normalizers.histogram_matching import HistogramMatching
from stainx_amd.normalizers.macenko import Macenko
from stainx_amd.normalizers.reinhard import Reinhard
from stainx_amd.normalizers.vahadane import Vahadane

__all__ = ["HistogramMatching", "Macenko", "Reinhard", "Vahadane"]
