// Luminosity standardisation (included at the end of reinhard.hip): the exact nearest-rank percentile of the luminance Y over a tile or
// a batch (sx_luminosity_percentile), and the one-launch map L*' = min(100 L* / L_p, 100) with a* and b* kept (sx_luminosity_apply).
// DESIGN.md 5i.
//
// The percentile: L* is monotone in Y, so the selection runs on Y = tissue::luminance() of the linear-light values -- the float32 every
// masked kernel compares -- and needs no cube root.  An exact radix selection on float_key(Y) with the bookkeeping of the percentile
// concentrations (radix_select.hpp: 11 / 11 / 10 bits): a memset, three streaming passes with integer histograms -- LDS atomics, then
// integer atomics to global memory -- each followed by a one-workgroup step that finds the bin of the wanted rank.  Integer sums only:
// exact, deterministic, a tile's row the same alone or in a batch, a pooled one-tile batch the bits of the tile's row.
// What differs from the concentrations: a slide is mostly glass, most pixels of a tile share ONE key, and one LDS word would take an
// atomic add per pixel from every lane in turn.  A lane therefore counts a run of equal bins itself and adds once per run (as
// level_histogram_kernel and luminosity_histogram_kernel do): on glass one add per lane and work item.
//
// The apply pass: apply_chunk's structure (reinhard.hip) without the a* / b* multiplies and without the codes -- f_y' = min(g f_y +
// (16/116)(1 - g), 1), the differences f_x - f_y and f_y - f_z kept -- with g = 100 / L_p formed once per workgroup in fp64 from the
// float32 percentile in device memory.
#pragma once

#include "radix_select.hpp"

namespace sx {
namespace luminosity {

using namespace sx::reinhard;
using radix::kBinsAll;
using radix::PassBins;
using radix::SelectState;

constexpr int kChunk = 16384;           // pixels per work item of a histogram pass: whole sweeps of 256 threads x 4 pixels
constexpr int kSelectThreads = 256;
static_assert(kChunk % (kStreamThreads * 4) == 0, "a work item is whole sweeps of packs");

struct Layout {
    size_t hist, select, total;
};
static Layout layout(int64_t n_tiles) {
    Layout l;
    l.hist = 0;
    l.select = align_up(sizeof(unsigned long long) * kBinsAll * (size_t)n_tiles, 256);
    l.total = l.select + align_up(sizeof(SelectState) * (size_t)n_tiles, 256);
    return l;
}

struct SelectArgs {
    unsigned long long* hist;      // rows x kBinsAll
    SelectState* select;           // rows
    const uint8_t* mask;           // (N, H*W) bytes, non-zero = in S; null: every pixel
    int64_t pixels;
    int blocks, pooled;
};

// kRuns: a lane adds once per run of equal bins (the product); without, once per pixel (the diagnostic build's comparison form)
template <typename T, int V, bool kMask, int kPass, bool kRuns>
__global__ __launch_bounds__(kStreamThreads) void percentile_histogram_kernel(const T* __restrict__ images, SelectArgs a) {
    constexpr int kBins = 1 << PassBins<kPass>::bits, kBelow = PassBins<kPass>::below;
    __shared__ uint32_t hist[kBins];
    __shared__ LinearTable table;
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const int64_t group = a.pooled ? 0 : tile;
    const int64_t p_begin = (int64_t)chunk_id * kChunk, p_end = min(p_begin + (int64_t)kChunk, a.pixels);
    const T* img = images + tile * 3 * a.pixels;
    for (int b = threadIdx.x; b < kBins; b += kStreamThreads) hist[b] = 0u;
    if constexpr (sizeof(T) == 1) table.fill();
    __syncthreads();
    uint32_t prefix = 0u;
    if constexpr (kPass > 0) prefix = a.select[group].prefix;
    uint32_t last = 0u, run = 0u;
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        float u[3][V], lin[V][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) load_for_lab<T, V>(img + c * a.pixels + p, u[c]);
        pack_to_lin<T, V>(u, &table, lin);
        uint32_t in = (1u << V) - 1u;
        if constexpr (kMask) in = tissue_bits<V>(tissue::Source{a.mask, 0.0f}, tile * a.pixels + p, lin);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float y = tissue::luminance(lin[i][0], lin[i][1], lin[i][2]);
            const uint32_t key = float_key(y);
            const uint32_t bin = (key >> kBelow) & (uint32_t)(kBins - 1);
            bool mine = ((in >> i) & 1u) && y == y;      // (a NaN is not in S: its key would sort on top and shift the rank)
            if constexpr (kPass > 0) mine = mine && (key >> (kBelow + PassBins<kPass>::bits)) == prefix;
            if (!mine) continue;
            if constexpr (kRuns) {
                if (bin == last) {
                    ++run;
                } else {
                    if (run) atomicAdd(&hist[last], run);
                    last = bin;
                    run = 1u;
                }
            } else {
                atomicAdd(&hist[bin], 1u);
            }
        }
    }
    if constexpr (kRuns) {
        if (run) atomicAdd(&hist[last], run);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kStreamThreads) {
        const uint32_t c = hist[b];
        if (c != 0u) atomicAdd(&a.hist[group * kBinsAll + PassBins<kPass>::offset + b], (unsigned long long)c);
    }
}

// One workgroup per row: the bin that holds the wanted rank.  Pass 0 also counts |S| and forms the rank, k = 1 + rint(fraction * (|S| - 1))
// with fraction = 0.01 * percentile, half to even, in doubles; pass 2 writes the percentile (NaN for an empty S) and |S|.
template <int kPass>
__global__ __launch_bounds__(kSelectThreads) void percentile_select_kernel(SelectArgs a, double fraction, float* __restrict__ luminance_out, unsigned long long* __restrict__ pixels_out) {
    constexpr int kBins = 1 << PassBins<kPass>::bits, kPer = kBins / kSelectThreads;
    __shared__ unsigned long long part[kSelectThreads];
    const int64_t row = blockIdx.x;
    const unsigned long long* hist = a.hist + row * kBinsAll + PassBins<kPass>::offset;
    unsigned long long mine = 0ull;
    for (int b = 0; b < kPer; ++b) mine += hist[threadIdx.x * kPer + b];
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    SelectState st;
    if constexpr (kPass == 0) {
        unsigned long long total = 0ull;
        for (int q = 0; q < kSelectThreads; ++q) total += part[q];
        st.count = total;
        st.rank = total ? 1ull + (unsigned long long)rint(fraction * (double)(total - 1ull)) : 0ull;
        st.prefix = 0u;
        st.pad = 0u;
    } else {
        st = a.select[row];
    }
    uint32_t bin = 0u;
    unsigned long long before = 0ull;
    if (st.count) {
        int q = 0;
        while (q < kSelectThreads - 1 && before + part[q] < st.rank) before += part[q++];
        int b = q * kPer;
        const int b_last = q * kPer + kPer - 1;
        while (b < b_last && before + hist[b] < st.rank) before += hist[b++];
        bin = (uint32_t)b;
    }
    st.rank -= before;
    st.prefix = (st.prefix << PassBins<kPass>::bits) | bin;
    a.select[row] = st;
    if constexpr (kPass == 2) {
        luminance_out[row] = st.count ? key_float(st.prefix) : __uint_as_float(0x7fc00000u);
        if (pixels_out) pixels_out[row] = st.count;
    }
}

// The apply pass.  Row 0 of `luminance` for every tile (per_tile == 0) or row `tile`.  A row that is NaN (S was empty), gives L_p <= 0 (a
// black tile) or is exactly 1 (the percentile is white already: gain 1, where the float32 round trip followed by the truncation to a level
// would take one level off about half the elements of a uint8 tile) copies its tiles through bit for bit: a workgroup-uniform branch.
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void standardize_kernel(const T* __restrict__ images, T* __restrict__ out, Geometry g, const float* __restrict__ luminance, int per_tile) {
    const int64_t tile = blockIdx.x / g.blocks_per_tile;
    const int chunk_id = blockIdx.x % g.blocks_per_tile;
    const int64_t p_begin = (int64_t)chunk_id * g.chunk, p_end = min(p_begin + g.chunk, g.pixels);
    const T* img = images + tile * 3 * g.pixels;
    T* dst = out + tile * 3 * g.pixels;
    __shared__ float map[2];
    __shared__ int copy_through;
    __shared__ LinearTable table;
    if (threadIdx.x == 0) {      // fp64, once per workgroup, from the float32 percentile
        const float y_f = luminance[per_tile ? tile : 0];
        const double y_p = (double)y_f;
        const double f_p = y_p > 0.008856 ? cbrt(y_p) : 7.787 * y_p + 16.0 / 116.0;
        const double l_p = 116.0 * f_p - 16.0;
        const bool through = !(y_f == y_f) || !(l_p > 0.0) || y_f == 1.0f;      // (Y_p = 1: L_p = 100, the gain is 1 and the map the identity)
        const double gain = through ? 1.0 : 100.0 / l_p;
        map[0] = (float)gain;
        map[1] = (float)((16.0 / 116.0) * (1.0 - gain));
        copy_through = through ? 1 : 0;
    }
    if constexpr (sizeof(T) == 1) table.fill();
    __syncthreads();
    if (copy_through) {
        for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Pack<T, V> pk;
                if constexpr (V == 1) pk.v[0] = img[c * g.pixels + p]; else pk = load_pack_stream<T, V>(img + c * g.pixels + p);
                store_pack_stream<T, V>(dst + c * g.pixels + p, pk.v);
            }
        }
        return;
    }
    const float gain = map[0], shift = map[1];
    const MatrixLane fwd = forward_matrix(), inv = inverse_matrix();
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        T res[3][V];
        float u[3][V], e[V][3], xyz[V][3], lin[V][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) load_for_lab_last<T, V>(img + c * g.pixels + p, u[c]);
        pack_to_e<T, V>(u, &table, fwd, e);      // e = (f_y, f_x - f_y, f_y - f_z)
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float fy = fminf(fmaf(gain, e[i][0], shift), 1.0f);      // L*' = min(g L*, 100)
            xyz[i][0] = f_inv(fy + e[i][1]);                               // a*, b* kept
            xyz[i][1] = f_inv(fy);
            xyz[i][2] = f_inv(fy - e[i][2]);
        }
        matrix_times_pack<V>(inv, xyz, lin);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float back[3];
            linear_to_rgb(lin[i], back);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (sizeof(T) == 1)
                    res[c][i] = Elem<T>::store(fminf(fmaxf(back[c] * 255.0f, 0.0f), 255.0f));
                else
                    res[c][i] = Elem<T>::store(back[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) store_pack_stream<T, V>(dst + c * g.pixels + p, res[c]);
    }
}

struct Call {
    const void* images;
    int dtype;
    int64_t n;
    bool vec;
    double fraction;
    hipStream_t stream;
};

template <typename T, int V, bool kMask, bool kRuns>
static void launch_passes(const Call& c, const SelectArgs& a, float* luminance_out, unsigned long long* pixels_out) {
    const unsigned grid = (unsigned)(c.n * a.blocks), rows = (unsigned)(a.pooled ? 1 : c.n);
    const T* img = static_cast<const T*>(c.images);
    hipLaunchKernelGGL((percentile_histogram_kernel<T, V, kMask, 0, kRuns>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a);
    hipLaunchKernelGGL(percentile_select_kernel<0>, dim3(rows), dim3(kSelectThreads), 0, c.stream, a, c.fraction, luminance_out, pixels_out);
    hipLaunchKernelGGL((percentile_histogram_kernel<T, V, kMask, 1, kRuns>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a);
    hipLaunchKernelGGL(percentile_select_kernel<1>, dim3(rows), dim3(kSelectThreads), 0, c.stream, a, c.fraction, luminance_out, pixels_out);
    hipLaunchKernelGGL((percentile_histogram_kernel<T, V, kMask, 2, kRuns>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a);
    hipLaunchKernelGGL(percentile_select_kernel<2>, dim3(rows), dim3(kSelectThreads), 0, c.stream, a, c.fraction, luminance_out, pixels_out);
}
template <typename T, bool kRuns>
static void passes_typed(const Call& c, const SelectArgs& a, float* luminance_out, unsigned long long* pixels_out) {
    if (a.mask) {
        if (c.vec) launch_passes<T, 4, true, kRuns>(c, a, luminance_out, pixels_out); else launch_passes<T, 1, true, kRuns>(c, a, luminance_out, pixels_out);
    } else {
        if (c.vec) launch_passes<T, 4, false, kRuns>(c, a, luminance_out, pixels_out); else launch_passes<T, 1, false, kRuns>(c, a, luminance_out, pixels_out);
    }
}

static size_t element_bytes(int dtype) { return dtype == SX_U8 ? 1 : dtype == SX_F16 || dtype == SX_BF16 ? 2 : dtype == SX_F32 ? 4 : 8; }
static bool sizes_overflow(int64_t n, int64_t h, int64_t w) { return n > 0x7fffffffll || h > 0x7fffffffll || w > 0x7fffffffll || h * w > (1ll << 40); }

// Every check, then a memset, three streaming passes and three one-workgroup steps on the stream.
template <bool kRuns>
static int run_percentile(const char* who, const void* images, int dtype, int64_t n, int64_t h, int64_t w, const uint8_t* mask, int pooled, double percentile, float* luminance_out,
                      unsigned long long* pixels_out, void* ws, size_t ws_bytes, void* stream) {
    if (!images) return fail(SX_ERR_BAD_ARG, "%s: images pointer is null", who);
    if (!luminance_out) return fail(SX_ERR_BAD_ARG, "%s: luminance_out pointer is null", who);
    if (dtype < SX_U8 || dtype > SX_F64) return fail(SX_ERR_DTYPE, "%s: unsupported dtype code %d", who, dtype);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "%s: n, h, w must be positive, got n=%lld h=%lld w=%lld", who, (long long)n, (long long)h, (long long)w);
    if (sizes_overflow(n, h, w)) return fail(SX_ERR_BAD_ARG, "%s: n, h, w overflow one call (n=%lld h=%lld w=%lld)", who, (long long)n, (long long)h, (long long)w);
    const int64_t pixels = h * w, blocks = (pixels + kChunk - 1) / kChunk;
    if (blocks > 0x7fffffffll / n) return fail(SX_ERR_BAD_ARG, "%s: n, h, w overflow one call: %lld work items", who, (long long)n * (long long)blocks);
    if (!(percentile > 0.0) || !(percentile <= 100.0)) return fail(SX_ERR_BAD_ARG, "%s: percentile must lie in (0, 100], got %g", who, percentile);
    const Layout l = layout(n);
    if (!ws || ws_bytes < l.total) return fail(SX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", who, l.total, ws ? ws_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(SX_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
    char* base = static_cast<char*>(ws);
    SelectArgs a;
    a.hist = reinterpret_cast<unsigned long long*>(base + l.hist);
    a.select = reinterpret_cast<SelectState*>(base + l.select);
    a.mask = mask;
    a.pixels = pixels;
    a.blocks = (int)blocks;
    a.pooled = pooled != 0;
    Call c;
    c.images = images;
    c.dtype = dtype;
    c.n = n;
    c.vec = pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (element_bytes(dtype) * 4) == 0 && (!mask || reinterpret_cast<uintptr_t>(mask) % 4 == 0);
    c.fraction = 0.01 * percentile;
    c.stream = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)(a.pooled ? 1 : n);
    if (hipMemsetAsync(a.hist, 0, sizeof(unsigned long long) * kBinsAll * rows, c.stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    switch (dtype) {
        case SX_U8: passes_typed<uint8_t, kRuns>(c, a, luminance_out, pixels_out); break;
        case SX_F16: passes_typed<__half, kRuns>(c, a, luminance_out, pixels_out); break;
        case SX_BF16: passes_typed<__hip_bfloat16, kRuns>(c, a, luminance_out, pixels_out); break;
        case SX_F32: passes_typed<float, kRuns>(c, a, luminance_out, pixels_out); break;
        default: passes_typed<double, kRuns>(c, a, luminance_out, pixels_out); break;
    }
    return check_launch("luminosity percentile");
}

}  // namespace luminosity
}  // namespace sx

extern "C" size_t sx_luminosity_workspace_bytes(int dtype, int64_t n, int64_t h, int64_t w) {
    (void)dtype;
    if (n <= 0 || h <= 0 || w <= 0 || sx::luminosity::sizes_overflow(n, h, w)) return 0;
    return sx::luminosity::layout(n).total;
}

extern "C" int sx_luminosity_percentile(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const uint8_t* mask_dev, int pooled, double percentile, float* luminance_out,
                                        unsigned long long* pixels_out, void* ws, size_t ws_bytes, void* stream) {
    return sx::luminosity::run_percentile<true>("sx_luminosity_percentile", images, dtype, n, h, w, mask_dev, pooled, percentile, luminance_out, pixels_out, ws, ws_bytes, stream);
}

#ifdef SX_DIAG
// the selection with one LDS add per pixel (no runs): what the run counting is measured against (tools/bench_luminosity.py)
extern "C" int sx_luminosity_percentile_plain(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const uint8_t* mask_dev, int pooled, double percentile,
                                              float* luminance_out, unsigned long long* pixels_out, void* ws, size_t ws_bytes, void* stream) {
    return sx::luminosity::run_percentile<false>("sx_luminosity_percentile_plain", images, dtype, n, h, w, mask_dev, pooled, percentile, luminance_out, pixels_out, ws, ws_bytes, stream);
}
#endif

extern "C" int sx_luminosity_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* luminance_dev, int64_t n_sources, void* stream_ptr) {
    using namespace sx::luminosity;
    if (!images || !out) return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: images / out pointer is null");
    if (!luminance_dev) return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: luminance pointer is null");
    if (dtype < SX_U8 || dtype > SX_F64) return fail(SX_ERR_DTYPE, "sx_luminosity_apply: unsupported dtype code %d", dtype);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: n, h, w must be positive, got n=%lld h=%lld w=%lld", (long long)n, (long long)h, (long long)w);
    if (sizes_overflow(n, h, w) || (h * w + kStreamThreads * 4 - 1) / (kStreamThreads * 4) > 0x7fffffffll / n)
        return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: n, h, w overflow one call (n=%lld h=%lld w=%lld)", (long long)n, (long long)h, (long long)w);
    if (n_sources != 1 && n_sources != n) return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: n_sources must be 1 or n_tiles (%lld), got %lld", (long long)n, (long long)n_sources);
    if (out == images) return fail(SX_ERR_BAD_ARG, "sx_luminosity_apply: out must not be images (the call is not in place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int per_tile = sx::rows_per_tile(n_sources, n);
    return run_one_launch("luminosity apply", dtype, images, out, n, h, w, nullptr, [&](auto v, auto* in, auto* dst, const Geometry& g, dim3 grid) {
        using T = std::remove_pointer_t<decltype(dst)>;
        hipLaunchKernelGGL((standardize_kernel<T, decltype(v)::value>), grid, dim3(kStreamThreads), 0, stream, in, dst, g, luminance_dev, per_tile);
    });
}
