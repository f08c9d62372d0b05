// Vahadane stain estimation (sx_vahadane_estimate) and the 99th-percentile concentrations of a GIVEN basis (sx_stain_max_concentrations):
// kernels, launchers and entry points, on the helpers of macenko.hip (LevelTables, od_of / l2_of, pinv_of_he, MaskArgs).  DESIGN.md 4p.
//
// The estimate: sparse non-negative matrix factorisation of the optical density with TWO atoms,
//     min  0.5 |V - W H|^2 + lambda |H|_1,     W (3,2) >= 0 with unit columns,  H (2,|S|) >= 0,
// run for a FIXED number of rounds (no early exit: no synchronisation, capturable, deterministic).  One round is two launches:
//   vahadane_moments_kernel   streams the pixels: per pixel the exact two-variable non-negative lasso in float32 (closed form), and the
//                             nine sums the dictionary step needs -- A = H H^T (3 distinct), B = V H^T (6) -- plus the pixel count, as
//                             per-thread float32 partials, reduced in fp64 within the wave (DPP, fixed order) and through LDS; ten
//                             doubles per work item (tile, chunk) into the workspace
//   vahadane_update_kernel    one workgroup per group: adds the group's partials in an order that depends on their NUMBER only, then
//                             one block-coordinate sweep of the dictionary update in fp64; W stays fp64 in the group's state
// No floating-point atomics anywhere.  The pixels a THREAD sums, and their order, depend on (tile, chunk, thread) only -- the scalar path
// (tiles that are not pack-aligned) visits the pixels of the packs the vector path would load -- so a tile's row has the same bits alone
// or in a batch, from an aligned or an unaligned view, and a pooled estimate of a one-tile batch has the bits of that tile's row.
//
// The percentiles: an exact radix selection on the order-preserving 32-bit key of the float32 concentration that
// sx_macenko_separate_apply(_masked) writes in own-basis mode (the same fold from the same six floats, the same per-pixel expression):
// three streaming passes with integer histograms of 11 / 11 / 10 bits per (group, stain) -- LDS atomics, then integer atomics to global
// memory -- each followed by a one-workgroup step that finds the bin of the wanted rank.  Integer sums: exact and deterministic.
#pragma once

#include "radix_select.hpp"

namespace sx {
namespace vahadane {

using namespace sx::macenko;
using radix::kBinsAll;      // (11 / 11 / 10 bits, 5120 counts per (group, stain): radix_select.hpp, shared with the luminosity percentile)
using radix::kBits0;
using radix::kBits1;
using radix::kBits2;
using radix::PassBins;
using radix::SelectState;

constexpr int kVChunk = 16384;        // pixels per work item: a multiple of kStreamThreads * 16 (the widest pack)
constexpr int kVals = 10;             // A00 A01 A11  B00 B01 B10 B11 B20 B21  count
constexpr int kStateDoubles = 8;      // W (3,2) row-major in fp64, two spare
constexpr int kUpdateThreads = 256;
constexpr int kUpdateRows = 16;       // the update step adds partials m, m + 16, ... per row, then the sixteen rows in order
static_assert(kVChunk % (kStreamThreads * 16) == 0, "a work item is whole sweeps of every pack width");

struct Layout {
    size_t state, partials, hist, select, total;
};
static Layout layout(int64_t n_tiles, int64_t pixels) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t blocks = (size_t)((pixels + kVChunk - 1) / kVChunk);
    Layout l;
    l.state = 0;
    l.partials = up(l.state + sizeof(double) * kStateDoubles * (size_t)n_tiles);
    l.hist = up(l.partials + sizeof(double) * kVals * blocks * (size_t)n_tiles);
    l.select = up(l.hist + sizeof(unsigned long long) * 2 * kBinsAll * (size_t)n_tiles);
    l.total = up(l.select + sizeof(SelectState) * 2 * (size_t)n_tiles);
    return l;
}

struct EstimateArgs {
    const float* init;        // n_init x 6 floats, (3,2) row-major; columns normalised here
    double* state;            // rows x kStateDoubles
    double* partials;         // (n_tiles * blocks) x kVals
    int64_t pixels, n_tiles;
    int blocks, pooled, init_per_row;
    float lambda;
};

// The dictionary at the start of round `round`: the given initial columns, normalised in fp64 (round 0), or the group's state.
__device__ __forceinline__ void current_w(const EstimateArgs& a, int64_t group, int round, double (&w)[6]) {
    if (round == 0) {
        const float* src = a.init + (a.init_per_row ? group * 6 : 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double x = (double)src[j], y = (double)src[2 + j], z = (double)src[4 + j];
            const double nrm = sqrt(x * x + y * y + z * z);
            const double inv = nrm > 0.0 ? 1.0 / nrm : 1.0;
            w[j] = x * inv;
            w[2 + j] = y * inv;
            w[4 + j] = z * inv;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = a.state[group * kStateDoubles + i];
    }
}

// The V pixels of the pack at pixel p, as raw values (uint8: the grey level's integer bits), and which of them count: inside the work
// item and masked in.  kVec: 16-byte packs (the tile is pack-aligned, every pack lies inside the work item); otherwise the same V pixels
// one by one.  Values of pixels that do not count are never used but through a select.
template <typename T, bool kVec, bool kMask>
__device__ __forceinline__ uint32_t load_group(const T* __restrict__ img, const uint8_t* __restrict__ msk, int64_t pixels, int64_t p, int64_t p_end, float (&u)[3][PackOf<T>::n]) {
    constexpr int V = PackOf<T>::n;
    if constexpr (kVec) {
        load_pixels<T, V, false, sizeof(T) == 1>(img, pixels, p, u);
        if constexpr (kMask) {
            MaskPack<V> mp;
            mp.load(msk + p);
            return mp.bits();
        } else {
            return (1u << V) - 1u;
        }
    } else {
        uint32_t bits = 0u;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool valid = p + i < p_end;
            bool in = valid;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float one[1] = {0.0f};
                if (valid) load_values<T, 1, sizeof(T) == 1>(img + c * pixels + p + i, one);
                u[c][i] = one[0];
            }
            if constexpr (kMask) in = valid && msk[valid ? p + i : p] != 0;
            bits |= (in ? 1u : 0u) << i;
        }
        return bits;
    }
}

template <typename T, bool kVec, bool kMask>
__global__ __launch_bounds__(kStreamThreads) void vahadane_moments_kernel(const T* __restrict__ images, EstimateArgs a, int round, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int V = PackOf<T>::n, kWaves = kStreamThreads / kWave;
    __shared__ LevelTables<T> tb;
    __shared__ double red[kWaves][kVals];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const uint8_t* msk = tile_mask(mk, tile, a.pixels);
    const int64_t p_begin = (int64_t)chunk_id * kVChunk;
    const int64_t p_end = min(p_begin + (int64_t)kVChunk, a.pixels);
    const T* img = images + tile * 3 * a.pixels;

    double wd[6];
    current_w(a, a.pooled ? 0 : tile, round, wd);
    float w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = (float)wd[i];
    const float lambda = a.lambda;
    const float g = fmaf(w[4], w[5], fmaf(w[2], w[3], w[0] * w[1]));
    const float d = 1.0f - g * g;
    const bool independent = d > 1e-6f;      // (atoms parallel: the two-atom candidate is skipped)
    const float inv_d = independent ? 1.0f / d : 0.0f;
    tb.fill();

    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
    uint32_t count = 0u;
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        float u[3][V];
        const uint32_t in_bits = load_group<T, kVec, kMask>(img, msk, a.pixels, p, p_end, u);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool in = in_mask(in_bits, i);
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = in ? od_of<T>(u[c][i], tb) : 0.0f;
            const float b1 = fmaf(w[4], v[2], fmaf(w[2], v[1], w[0] * v[0])) - lambda;
            const float b2 = fmaf(w[5], v[2], fmaf(w[3], v[1], w[1] * v[0])) - lambda;
            const float r1 = fmaf(-g, b2, b1), r2 = fmaf(-g, b1, b2);      // b1 - g b2,  b2 - g b1
            const float c1 = r1 * inv_d, c2 = r2 * inv_d;
            float h1, h2;
            if (independent && c1 > 0.0f && c2 > 0.0f) {
                h1 = c1;
                h2 = c2;
            } else if (b1 > 0.0f && r2 <= 0.0f) {
                h1 = b1;
                h2 = 0.0f;
            } else if (b2 > 0.0f) {
                h1 = 0.0f;
                h2 = b2;
            } else {
                h1 = h2 = 0.0f;
            }
            h1 = in ? h1 : 0.0f;
            h2 = in ? h2 : 0.0f;
            acc[0] = fmaf(h1, h1, acc[0]);
            acc[1] = fmaf(h1, h2, acc[1]);
            acc[2] = fmaf(h2, h2, acc[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[3 + 2 * c] = fmaf(v[c], h1, acc[3 + 2 * c]);
                acc[4 + 2 * c] = fmaf(v[c], h2, acc[4 + 2 * c]);
            }
            count += in ? 1u : 0u;
        }
    }
    // wave (DPP, fixed order, total in lane 63) -> LDS -> one sum per value in wave order
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    double vals[kVals];
#pragma unroll
    for (int k = 0; k < 9; ++k) vals[k] = (double)acc[k];
    vals[9] = (double)count;
#pragma unroll
    for (int k = 0; k < kVals; ++k) {
        const double total = wave_total_f64(vals[k]);
        if (lane == kWave - 1) red[wave][k] = total;
    }
    __syncthreads();
    if (threadIdx.x < kVals) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < kWaves; ++v) s += red[v][threadIdx.x];
        a.partials[(int64_t)blockIdx.x * kVals + threadIdx.x] = s;
    }
}

// One workgroup per group.  Thread (row r, value k) adds partials r, r + 16, ... of value k; thread 0 adds the sixteen rows in order:
// the order is a function of the number of partials alone.  Then the sweep, in fp64, by thread 0.
__global__ __launch_bounds__(kUpdateThreads) void vahadane_update_kernel(EstimateArgs a, int round, int last, float* __restrict__ he_out, unsigned long long* __restrict__ pixels_out) {
    __shared__ double rows[kUpdateRows][16];
    const int64_t group = blockIdx.x;
    const int64_t count = a.pooled ? a.n_tiles * a.blocks : a.blocks;
    const double* base = a.partials + (a.pooled ? 0 : group * a.blocks * kVals);
    const int k = threadIdx.x % 16, r = threadIdx.x / 16;
    double s = 0.0;
    if (k < kVals)
        for (int64_t m = r; m < count; m += kUpdateRows) s += base[m * kVals + k];
    rows[r][k] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[kVals];
    for (int v = 0; v < kVals; ++v) {
        double sum = rows[0][v];
        for (int q = 1; q < kUpdateRows; ++q) sum += rows[q][v];
        t[v] = sum;
    }
    double w[6];
    current_w(a, group, round, w);
    const double A[2][2] = {{t[0], t[1]}, {t[1], t[2]}};
    for (int j = 0; j < 2; ++j) {
        if (!(A[j][j] > 0.0)) continue;      // an atom no pixel uses keeps its column
        double u[3], nrm2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double wa = w[c * 2] * A[0][j] + w[c * 2 + 1] * A[1][j];
            u[c] = fmax(w[c * 2 + j] + (t[3 + 2 * c + j] - wa) / A[j][j], 0.0);
            nrm2 += u[c] * u[c];
        }
        const double nrm = sqrt(nrm2);
        if (!(nrm > 0.0)) continue;
        for (int c = 0; c < 3; ++c) w[c * 2 + j] = u[c] / nrm;
    }
    for (int i = 0; i < 6; ++i) a.state[group * kStateDoubles + i] = w[i];
    if (last) {
        const bool swap = w[0] < w[1];      // haematoxylin: the column with the larger red optical density
        const bool empty = !(t[9] > 0.0);
        for (int c = 0; c < 3; ++c) {
            const float h = (float)(swap ? w[c * 2 + 1] : w[c * 2]), e = (float)(swap ? w[c * 2] : w[c * 2 + 1]);
            he_out[group * 6 + c * 2] = empty ? __uint_as_float(0x7fc00000u) : h;
            he_out[group * 6 + c * 2 + 1] = empty ? __uint_as_float(0x7fc00000u) : e;
        }
        if (pixels_out) pixels_out[group] = (unsigned long long)t[9];
    }
}

// ---- percentiles of the concentrations of a given basis ---------------------------------------------------------------------------
struct MaxcArgs {
    const float* he;                  // n_sources x 6
    unsigned long long* hist;         // rows x 2 x kBinsAll
    SelectState* select;              // rows x 2
    int64_t pixels, n_tiles;
    int blocks, pooled, per_row;
};

template <typename T, bool kVec, bool kMask, int kPass>
__global__ __launch_bounds__(kStreamThreads) void maxc_histogram_kernel(const T* __restrict__ images, MaxcArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int V = PackOf<T>::n, kBins = 1 << PassBins<kPass>::bits, kBelow = PassBins<kPass>::below;
    __shared__ LevelTables<T> tb;
    __shared__ uint32_t hist[2][kBins];
    __shared__ float fold[8];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const int64_t group = a.pooled ? 0 : tile;
    const uint8_t* msk = tile_mask(mk, tile, a.pixels);
    const int64_t p_begin = (int64_t)chunk_id * kVChunk;
    const int64_t p_end = min(p_begin + (int64_t)kVChunk, a.pixels);
    const T* img = images + tile * 3 * a.pixels;
    for (int b = threadIdx.x; b < 2 * kBins; b += kStreamThreads) (&hist[0][0])[b] = 0u;
    if (threadIdx.x == 0) {      // separate_apply_kernel's fold in own-basis mode (scale 1): a (2,3), b (2)
        const float* he_src = a.he + (a.per_row ? group * 6 : 0);
        float he[6], rec[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) he[i] = he_src[i];
        pinv_of_he(he, rec);
        double pinv[6];
        const double s = 1.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) pinv[i] = (double)rec[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) fold[3 * i + j] = (float)(-0.69314718055994530942 * s * pinv[3 * i + j]);      // ln 2
            fold[6 + i] = (float)(5.48063892334199 * s * (pinv[3 * i] + pinv[3 * i + 1] + pinv[3 * i + 2]));      // ln 240
        }
    }
    tb.fill();
    __syncthreads();
    float ca[2][3], cb[2];
    uint32_t prefix[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) ca[i][j] = fold[3 * i + j];
        cb[i] = fold[6 + i];
        if constexpr (kPass > 0) prefix[i] = a.select[group * 2 + i].prefix;
    }
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        float u[3][V];
        const uint32_t in_bits = load_group<T, kVec, kMask>(img, msk, a.pixels, p, p_end, u);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (!in_mask(in_bits, i)) continue;
            float l[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) l[c] = l2_of<T>(u[c][i], tb);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float v = fmaf(ca[s][2], l[2], fmaf(ca[s][1], l[1], fmaf(ca[s][0], l[0], cb[s])));
                const uint32_t key = float_key(v);
                const uint32_t bin = (key >> kBelow) & (uint32_t)(kBins - 1);
                bool mine = true;
                if constexpr (kPass > 0) mine = (key >> (kBelow + PassBins<kPass>::bits)) == prefix[s];
                if (mine) atomicAdd(&hist[s][bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * kBins; b += kStreamThreads) {
        const uint32_t c = (&hist[0][0])[b];
        if (c != 0u) atomicAdd(&a.hist[(group * 2 + b / kBins) * kBinsAll + PassBins<kPass>::offset + b % kBins], (unsigned long long)c);
    }
}

// One workgroup per (group, stain): the bin that holds the wanted rank.  Pass 0 also counts |S| and forms the rank,
// k = 1 + round(0.01 * 99 * (|S| - 1)), half to even; pass 2 writes the percentile (NaN for an empty group).
template <int kPass>
__global__ __launch_bounds__(kUpdateThreads) void maxc_select_kernel(MaxcArgs a, float* __restrict__ max_c_out, unsigned long long* __restrict__ pixels_out) {
    constexpr int kBins = 1 << PassBins<kPass>::bits, kPer = kBins / kUpdateThreads;
    __shared__ unsigned long long part[kUpdateThreads];
    const int64_t slot = blockIdx.x;      // group * 2 + stain
    const unsigned long long* hist = a.hist + slot * kBinsAll + PassBins<kPass>::offset;
    unsigned long long mine = 0ull;
    for (int b = 0; b < kPer; ++b) mine += hist[threadIdx.x * kPer + b];
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    SelectState st = a.select[slot];
    if constexpr (kPass == 0) {
        unsigned long long total = 0ull;
        for (int q = 0; q < kUpdateThreads; ++q) total += part[q];
        st.count = total;
        st.rank = total ? 1ull + (unsigned long long)rint((0.01 * 99.0) * (double)(total - 1ull)) : 0ull;
        st.prefix = 0u;
        st.pad = 0u;
    }
    uint32_t bin = 0u;
    unsigned long long before = 0ull;
    if (st.count) {
        int q = 0;
        while (q < kUpdateThreads - 1 && before + part[q] < st.rank) before += part[q++];
        int b = q * kPer;
        const int b_last = q * kPer + kPer - 1;
        while (b < b_last && before + hist[b] < st.rank) before += hist[b++];
        bin = (uint32_t)b;
    }
    st.rank -= before;
    st.prefix = (st.prefix << PassBins<kPass>::bits) | bin;
    a.select[slot] = st;
    if constexpr (kPass == 2) {
        max_c_out[slot] = st.count ? key_float(st.prefix) : __uint_as_float(0x7fc00000u);
        if (pixels_out && slot % 2 == 0) pixels_out[slot / 2] = st.count;
    }
}

struct Call {
    const void* images;
    const uint8_t* mask;
    int dtype;
    int64_t n, pixels;
    int blocks, pooled;
    bool vec;
    hipStream_t stream;
};

template <typename T, bool kVec, bool kMask>
static void launch_rounds(const Call& c, const EstimateArgs& a, int iterations, float* he_out, unsigned long long* pixels_out) {
    const unsigned grid = (unsigned)(c.n * c.blocks), rows = (unsigned)(c.pooled ? 1 : c.n);
    MaskArgs<kMask> mk;
    if constexpr (kMask) mk.mask = c.mask;
    for (int round = 0; round < iterations; ++round) {
        hipLaunchKernelGGL((vahadane_moments_kernel<T, kVec, kMask>), dim3(grid), dim3(kStreamThreads), 0, c.stream, static_cast<const T*>(c.images), a, round, mk);
        hipLaunchKernelGGL(vahadane_update_kernel, dim3(rows), dim3(kUpdateThreads), 0, c.stream, a, round, round == iterations - 1 ? 1 : 0, he_out, pixels_out);
    }
}

template <typename T, bool kVec, bool kMask>
static void launch_maxc(const Call& c, const MaxcArgs& a, float* max_c_out, unsigned long long* pixels_out) {
    const unsigned grid = (unsigned)(c.n * c.blocks), slots = (unsigned)(c.pooled ? 2 : 2 * c.n);
    MaskArgs<kMask> mk;
    if constexpr (kMask) mk.mask = c.mask;
    const T* img = static_cast<const T*>(c.images);
    hipLaunchKernelGGL((maxc_histogram_kernel<T, kVec, kMask, 0>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a, mk);
    hipLaunchKernelGGL(maxc_select_kernel<0>, dim3(slots), dim3(kUpdateThreads), 0, c.stream, a, max_c_out, pixels_out);
    hipLaunchKernelGGL((maxc_histogram_kernel<T, kVec, kMask, 1>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a, mk);
    hipLaunchKernelGGL(maxc_select_kernel<1>, dim3(slots), dim3(kUpdateThreads), 0, c.stream, a, max_c_out, pixels_out);
    hipLaunchKernelGGL((maxc_histogram_kernel<T, kVec, kMask, 2>), dim3(grid), dim3(kStreamThreads), 0, c.stream, img, a, mk);
    hipLaunchKernelGGL(maxc_select_kernel<2>, dim3(slots), dim3(kUpdateThreads), 0, c.stream, a, max_c_out, pixels_out);
}

template <typename T>
static void rounds_typed(const Call& c, const EstimateArgs& a, int iterations, float* he_out, unsigned long long* pixels_out) {
    if (c.mask) {
        if (c.vec) launch_rounds<T, true, true>(c, a, iterations, he_out, pixels_out); else launch_rounds<T, false, true>(c, a, iterations, he_out, pixels_out);
    } else {
        if (c.vec) launch_rounds<T, true, false>(c, a, iterations, he_out, pixels_out); else launch_rounds<T, false, false>(c, a, iterations, he_out, pixels_out);
    }
}
template <typename T>
static void maxc_typed(const Call& c, const MaxcArgs& a, float* max_c_out, unsigned long long* pixels_out) {
    if (c.mask) {
        if (c.vec) launch_maxc<T, true, true>(c, a, max_c_out, pixels_out); else launch_maxc<T, false, true>(c, a, max_c_out, pixels_out);
    } else {
        if (c.vec) launch_maxc<T, true, false>(c, a, max_c_out, pixels_out); else launch_maxc<T, false, false>(c, a, max_c_out, pixels_out);
    }
}

static int pack_width(int dtype) { return 16 / elem_bytes(dtype); }

// What both entry points check about the images, the mask, the flags and the workspace; fills `c`.  Nothing is enqueued.
static int prepare(const char* who, const void* images, int dtype, int64_t n, int64_t h, int64_t w, const unsigned char* mask, int pooled, unsigned flags, const void* ws, size_t ws_bytes, void* stream,
                   Call* c, Layout* l) {
    if (!images) return fail(SX_ERR_BAD_ARG, "%s: images pointer is null", who);
    if (dtype < SX_U8 || dtype > SX_F64) return fail(SX_ERR_DTYPE, "%s: unsupported dtype code %d", who, dtype);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "%s: n, h, w must be positive, got n=%lld h=%lld w=%lld", who, (long long)n, (long long)h, (long long)w);
    if (n > 0x7fffffffll || h > 0x7fffffffll || w > 0x7fffffffll || h * w > (1ll << 40)) return fail(SX_ERR_BAD_ARG, "%s: n, h, w overflow one call (n=%lld h=%lld w=%lld)", who, (long long)n, (long long)h, (long long)w);
    const int64_t pixels = h * w, blocks = (pixels + kVChunk - 1) / kVChunk;
    if (blocks > 0x7fffffffll / n) return fail(SX_ERR_BAD_ARG, "%s: n, h, w overflow one call: %lld work items", who, (long long)n * (long long)blocks);
    if (flags & ~SX_MACENKO_CLASSIC) return fail(SX_ERR_BAD_ARG, "%s: flags 0x%x: planar (N,3,H,W) tiles only, SX_MACENKO_CLASSIC (a no-op) is the one flag taken", who, flags);
    *l = layout(n, pixels);
    if (!ws || ws_bytes < l->total) return fail(SX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", who, l->total, ws ? ws_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(SX_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
    const int v = pack_width(dtype);
    c->images = images;
    c->mask = mask;
    c->dtype = dtype;
    c->n = n;
    c->pixels = pixels;
    c->blocks = (int)blocks;
    c->pooled = pooled != 0;
    c->vec = pixels % v == 0 && reinterpret_cast<uintptr_t>(images) % 16 == 0 && (!mask || reinterpret_cast<uintptr_t>(mask) % (uintptr_t)v == 0);
    c->stream = static_cast<hipStream_t>(stream);
    return SX_OK;
}

static int enqueue_maxc(const Call& c, const Layout& l, void* ws, const float* he, int per_row, float* max_c_out, unsigned long long* pixels_out) {
    char* base = static_cast<char*>(ws);
    const size_t rows = (size_t)(c.pooled ? 1 : c.n);
    MaxcArgs a;
    a.he = he;
    a.hist = reinterpret_cast<unsigned long long*>(base + l.hist);
    a.select = reinterpret_cast<SelectState*>(base + l.select);
    a.pixels = c.pixels;
    a.n_tiles = c.n;
    a.blocks = c.blocks;
    a.pooled = c.pooled;
    a.per_row = per_row;
    if (hipMemsetAsync(a.hist, 0, sizeof(unsigned long long) * 2 * kBinsAll * rows, c.stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    with_dtype(c.dtype, [&](auto t) { return maxc_typed<typename decltype(t)::type>(c, a, max_c_out, pixels_out), (int)SX_OK; });      // (prepare() has checked the code)
    return check_launch("stain max concentrations");
}

}  // namespace vahadane
}  // namespace sx

extern "C" size_t sx_vahadane_workspace_bytes(int dtype, int64_t n, int64_t h, int64_t w) {
    (void)dtype;
    if (n <= 0 || h <= 0 || w <= 0 || n > 0x7fffffffll || h > 0x7fffffffll || w > 0x7fffffffll || h * w > (1ll << 40)) return 0;
    return sx::vahadane::layout(n, h * w).total;
}

extern "C" int sx_vahadane_estimate(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const unsigned char* mask_dev, int pooled, const float* init_he, int64_t n_init, double lambda,
                                    int iterations, float* he_out, float* max_c_out, unsigned long long* pixels_out, unsigned flags, void* ws_ptr, size_t ws_bytes, void* stream_ptr) {
    using namespace sx::vahadane;
    Call c;
    Layout l;
    if (!init_he) return fail(SX_ERR_BAD_ARG, "sx_vahadane_estimate: init_he pointer is null");
    if (!he_out) return fail(SX_ERR_BAD_ARG, "sx_vahadane_estimate: he_out pointer is null");
    if (iterations < 1 || iterations > 1000) return fail(SX_ERR_BAD_ARG, "sx_vahadane_estimate: iterations must lie in 1..1000, got %d", iterations);
    if (!(lambda >= 0.0) || !(lambda <= 3.0e38)) return fail(SX_ERR_BAD_ARG, "sx_vahadane_estimate: lambda must be finite and not negative, got %g", lambda);
    int rc = prepare("sx_vahadane_estimate", images, dtype, n, h, w, mask_dev, pooled, flags, ws_ptr, ws_bytes, stream_ptr, &c, &l);
    if (rc != SX_OK) return rc;
    const int64_t rows = c.pooled ? 1 : n;
    if (n_init != 1 && n_init != rows) return fail(SX_ERR_BAD_ARG, "sx_vahadane_estimate: n_init must be 1 or the number of rows (%lld), got %lld", (long long)rows, (long long)n_init);
    char* base = static_cast<char*>(ws_ptr);
    EstimateArgs a;
    a.init = init_he;
    a.state = reinterpret_cast<double*>(base + l.state);
    a.partials = reinterpret_cast<double*>(base + l.partials);
    a.pixels = c.pixels;
    a.n_tiles = n;
    a.blocks = c.blocks;
    a.pooled = c.pooled;
    a.init_per_row = n_init != 1 ? 1 : 0;
    a.lambda = (float)lambda;
    with_dtype(dtype, [&](auto t) { return rounds_typed<typename decltype(t)::type>(c, a, iterations, he_out, pixels_out), (int)SX_OK; });      // (prepare() has checked the code)
    rc = check_launch("vahadane estimate");
    if (rc != SX_OK || !max_c_out) return rc;
    return enqueue_maxc(c, l, ws_ptr, he_out, 1, max_c_out, nullptr);
}

extern "C" int sx_stain_max_concentrations(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const unsigned char* mask_dev, int pooled, const float* he_dev, int64_t n_sources,
                                           float* max_c_out, unsigned long long* pixels_out, unsigned flags, void* ws_ptr, size_t ws_bytes, void* stream_ptr) {
    using namespace sx::vahadane;
    Call c;
    Layout l;
    if (!he_dev) return fail(SX_ERR_BAD_ARG, "sx_stain_max_concentrations: he pointer is null");
    if (!max_c_out) return fail(SX_ERR_BAD_ARG, "sx_stain_max_concentrations: max_c_out pointer is null");
    int rc = prepare("sx_stain_max_concentrations", images, dtype, n, h, w, mask_dev, pooled, flags, ws_ptr, ws_bytes, stream_ptr, &c, &l);
    if (rc != SX_OK) return rc;
    const int64_t rows = c.pooled ? 1 : n;
    if (n_sources != 1 && n_sources != rows) return fail(SX_ERR_BAD_ARG, "sx_stain_max_concentrations: n_sources must be 1 or the number of rows (%lld), got %lld", (long long)rows, (long long)n_sources);
    return enqueue_maxc(c, l, ws_ptr, he_dev, n_sources != 1 ? 1 : 0, max_c_out, pixels_out);
}
