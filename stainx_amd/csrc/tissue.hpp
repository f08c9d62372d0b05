// The tissue rule shared by every masked kernel (Reinhard statistics and apply, histogram matching, sx_tissue_mask): ONE device
// function, so that all paths agree on every pixel bit for bit.
//
// Rule (staintools' LuminosityThresholdTissueLocator, tiatoolbox): a pixel is tissue iff L* / 100 < luminosity_threshold, L* of the
// pixel's unit value.  L* = 116 f(Y) - 16 is monotone in the linear-light luminance Y, so the test is a comparison of Y with a
// constant derived on the host -- three multiply-adds on the linear-light values the Reinhard passes already hold, no cube root.
#pragma once

#include "common.hpp"

namespace sx {

// pow through v_log_f32 / v_exp_f32; x > 0.  The BARE instructions: every pow whose result is used has a normal argument and a normal
// result (colour values and their powers are >= 3e-3), and the range handling of exp2f / __log2f -- compare, select, rescale: ~8
// instructions per pow, nine pows per pixel in the Reinhard apply pass -- only matters for denormals (apply 689 -> 526 vector
// instructions per four pixels; 146 -> 130 us per call, max error against the oracle unchanged at 1.2e-5,
// tools/check_reinhard_error.py).  A branch that is not taken may see log(0) or log(negative): its value is dropped.
__device__ __forceinline__ float fast_pow(float x, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)); }

// (The piecewise functions stay `cond ? pow : line`: the compiler keeps an exec-mask branch around each logarithm / exponential pair,
// six per pixel in the apply pass.  Computing both pieces and selecting removes 170 scalar instructions and 50 s_nop per four pixels
// and is no faster -- 134 against 130 us per call: both passes are bound by the vector instruction count, 448 per four pixels of which
// 70 are quarter-rate logarithms / exponentials, and the select form has nine more.)
__device__ __forceinline__ float srgb_to_linear(float v) {      // torch_backend.py:28-29
    return v > 0.04045f ? fast_pow((v + 0.055f) * (1.0f / 1.055f), 2.4f) : v * (1.0f / 12.92f);
}

// uint8 pixels take one of 256 values per channel: their linear-light value comes from a table in LDS (filled with the very
// expression above, so every pixel gets the bits it got before) instead of a division, a logarithm and an exponential each.
struct LinearTable {
    float lin[256];
    __device__ __forceinline__ void fill() {
        for (int t = threadIdx.x; t < 256; t += blockDim.x) lin[t] = srgb_to_linear(Elem<uint8_t>::load((uint8_t)t));
        __syncthreads();
    }
};

namespace tissue {

// What a masked kernel is handed: an explicit mask (N x H x W bytes, non-zero = tissue) or, with mask == nullptr, the rule's constant.
struct Source {
    const uint8_t* mask;
    float y_cut;
};

// THE rule: linear-light R, G, B (of the unit value: the table for uint8, srgb_to_linear() otherwise) -> tissue or not.  Y by the
// colour conversion's middle row (torch_backend.py:32); a NaN pixel is background.
__device__ __forceinline__ float luminance(float lin_r, float lin_g, float lin_b) {      // (also what the luminosity histogram bins: tissue_detect.hpp)
    return fmaf(0.072169f, lin_b, fmaf(0.715160f, lin_g, 0.212671f * lin_r));
}
__device__ __forceinline__ bool is_tissue(float lin_r, float lin_g, float lin_b, float y_cut) {
    return luminance(lin_r, lin_g, lin_b) < y_cut;
}

// linear-light value of one stored element, as the Reinhard passes compute it
template <typename T>
__device__ __forceinline__ float linear_of(T v, const LinearTable& table) {
    if constexpr (sizeof(T) == 1) return table.lin[(int)v]; else return srgb_to_linear(Elem<T>::load(v));
}

// host: L* / 100 < threshold  <=>  Y < y_cut  (f(Y) = (L* + 16) / 116, inverted piecewise as the conversion's f, torch_backend.py:41-42)
inline bool threshold_ok(double threshold) { return threshold > 0.0 && threshold < 1.0; }
inline float y_cut_of(double threshold) {
    const double f = (100.0 * threshold + 16.0) / 116.0;
    return (float)(f * f * f > 0.008856 ? f * f * f : (f - 16.0 / 116.0) / 7.787);
}
// the masked entry points: an explicit mask, or the rule with a threshold in range
inline int check_source(const uint8_t* mask, double threshold) {
    if (!mask && !threshold_ok(threshold)) return fail(SX_ERR_BAD_ARG, "luminosity_threshold must lie in (0, 1), got %g", threshold);
    return SX_OK;
}
inline Source source_of(const uint8_t* mask, double threshold) { return Source{mask, mask ? 0.0f : y_cut_of(threshold)}; }

}  // namespace tissue
}  // namespace sx
