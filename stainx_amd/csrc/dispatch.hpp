// Host-side dispatch rules of libstainx_hip: every runtime decision that picks a template instantiation -- the element type of a call,
// the output element of the Macenko / deconvolution calls, pack width and layout -- is written once, here.  Host-only templates: the
// kernels a caller's lambda names are instantiated for exactly the (type, flag) pairs a rule calls it with, so a rule must not reach a
// pair the library has no kernel for (the uint8-only output elements stay behind `if constexpr (sizeof(T) == 1)`).
#pragma once

#include <type_traits>

#include "common.hpp"

namespace sx {

template <typename T> struct Tag { using type = T; };
template <int N> using int_constant = std::integral_constant<int, N>;

// The one five-way switch on a dtype code (SX_U8 ... SX_F64): f(Tag<T>{}).
template <typename F>
static int with_dtype(int dtype, F&& f) {
    switch (dtype) {
        case SX_U8: return f(Tag<uint8_t>{});
        case SX_F16: return f(Tag<__half>{});
        case SX_BF16: return f(Tag<__hip_bfloat16>{});
        case SX_F32: return f(Tag<float>{});
        case SX_F64: return f(Tag<double>{});
        default: return fail(SX_ERR_DTYPE, "unsupported dtype code %d", dtype);
    }
}
// (a check of its own, for the calls that enqueue something before they dispatch)
static inline int dtype_ok(int dtype) { return with_dtype(dtype, [](auto) { return (int)SX_OK; }); }

static inline int elem_bytes(int dtype) { return dtype == SX_U8 ? 1 : (dtype == SX_F16 || dtype == SX_BF16) ? 2 : dtype == SX_F32 ? 4 : 8; }

// ---- the output element of the calls that take SX_MACENKO_OUT_BF16 / _OUT_F16 / _NORMALIZE_0_1 --------------------------------
// uint8 input: bfloat16 or float16 where asked for (an extension: SURVEY.md 8f-2), float32 with the fused / 255, uint8 otherwise;
// every other input: its own element.  A call without an image output (concentrations only) runs with float.
static inline int out_code_of(unsigned flags) { return (flags & SX_MACENKO_OUT_BF16) ? SX_BF16 : ((flags & SX_MACENKO_OUT_F16) ? SX_F16 : 0); }
static inline int out_flags_ok(unsigned flags, int dtype) {
    if ((flags & (SX_MACENKO_OUT_BF16 | SX_MACENKO_OUT_F16)) != 0 && (dtype != SX_U8 || (flags & SX_MACENKO_OUT_BF16 && flags & SX_MACENKO_OUT_F16)))
        return fail(SX_ERR_BAD_ARG, "SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16: uint8 input only, one of the two");
    return SX_OK;
}
static inline size_t out_elem_bytes(int in_elem, int out_code, bool unit, bool has_image = true) {
    if (!has_image) return sizeof(float);
    return (in_elem == 1 && out_code != 0) ? 2 : ((in_elem == 1 && unit) ? sizeof(float) : (size_t)in_elem);
}
// f(Tag<O>{}, std::bool_constant<U>{}) -- O the output element, U the fused / 255 -- for exactly the pairs the library has kernels for:
// uint8 input (bf16, t/f), (f16, t/f), (float, true), (uint8, false); every other input (T, t/f).
template <typename T, typename F>
static int with_out(int out_code, bool unit, F&& f) {
    if constexpr (sizeof(T) == 1) {
        if (out_code == SX_BF16) return unit ? f(Tag<__hip_bfloat16>{}, std::true_type{}) : f(Tag<__hip_bfloat16>{}, std::false_type{});
        if (out_code != 0) return unit ? f(Tag<__half>{}, std::true_type{}) : f(Tag<__half>{}, std::false_type{});
        return unit ? f(Tag<float>{}, std::true_type{}) : f(Tag<T>{}, std::false_type{});
    } else {
        return unit ? f(Tag<T>{}, std::true_type{}) : f(Tag<T>{}, std::false_type{});
    }
}
// (the separations: !has_image -- concentrations only -- is (float, false))
template <typename T, typename F>
static int with_out(int out_code, bool unit, bool has_image, F&& f) {
    if (!has_image) return f(Tag<float>{}, std::false_type{});
    return with_out<T>(out_code, unit, f);
}

// ---- packs ----------------------------------------------------------------------------------------------------------------------
// The passes that write images are paced by their stores: their pack is 16 bytes of OUTPUT per lane and plane, so that one store
// instruction of a wave writes 1 KB of consecutive bytes.  With the input's pack (16 pixels per lane for uint8) a wider output
// type leaves every lane 64-192 bytes of its own and every store instruction 64 different lines: uint8 -> float32 (/255)
// took 172 us planar and 569 us NHWC for the config-2 batch where the same-width uint8 output takes 24 us.
template <typename O, int V>
constexpr int pack_for() { return V == 1 ? 1 : ((int)(16 / sizeof(O)) < V ? (int)(16 / sizeof(O)) : V); }

// f(int_constant<W or 1>{}, std::bool_constant<kInter>{}): 16-byte packs or single pixels, (N,H,W,3) or planar tiles.  kPlanarOnly (the
// masked calls): kInter = true is never instantiated.
template <int W, bool kPlanarOnly = false, typename F>
static int with_layout(bool vec, bool interleaved, F&& f) {
    if constexpr (!kPlanarOnly) {
        if (interleaved) return vec ? f(int_constant<W>{}, std::true_type{}) : f(int_constant<1>{}, std::true_type{});
    }
    return vec ? f(int_constant<W>{}, std::false_type{}) : f(int_constant<1>{}, std::false_type{});
}

// f(std::bool_constant<a>{}, std::bool_constant<b>{}): two flags of a kernel (packs x channels-last, packs x per tile), all four pairs;
// what f returns (a launch: nothing).
template <typename F>
static auto with_flags(bool a, bool b, F&& f) {
    if (a) return b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// ---- argument checks the entry points share ---------------------------------------------------------------------------------------
static inline int check_tiles(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must be (N,3,H,W) with positive sizes, got N=%lld H=%lld W=%lld", (long long)n, (long long)h, (long long)w);
    if (n * h * w >= (1ll << 32)) return fail(SX_ERR_BAD_ARG, "N*H*W must be below 2^32 pixels");
    return SX_OK;
}
// (the Reinhard and the histogram-matching calls: their own two texts, and no limit on the pixels of a call)
static inline int check_sizes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must be (N,3,H,W) with positive sizes");
    return SX_OK;
}
static inline int check_sizes_got(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes, got N=%lld H=%lld W=%lld", (long long)n, (long long)h, (long long)w);
    return SX_OK;
}
// rows given per call: one for the batch, or one per tile
static inline int check_rows(const char* name, int64_t rows, int64_t n) {
    if (rows != 1 && rows != n) return fail(SX_ERR_BAD_ARG, "%s must be 1 or n_tiles (%lld), got %lld", name, (long long)n, (long long)rows);
    return SX_OK;
}
static inline int rows_per_tile(int64_t rows, int64_t n) { return rows == n && n != 1 ? 1 : 0; }
static inline int check_workspace(const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need) return fail(SX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(SX_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    return SX_OK;
}
static inline int check_mask(const void* mask) {
    if (!mask) return fail(SX_ERR_BAD_ARG, "mask pointer is null (the masked calls take explicit masks: one byte per pixel, (N, H, W))");
    return SX_OK;
}

}  // namespace sx
