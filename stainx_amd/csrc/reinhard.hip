// Reinhard LAB statistics matching for MI355X (gfx950).
//
// Numerics follow ReinhardTorch (rendeirolab/stainx src/stainx/backends/torch_backend.py:17-101,
// 304-355): sRGB -> linear -> XYZ/D65 -> scaled LAB, mean / unbiased std pooled over the WHOLE batch
// (N,H,W), (lab-mu)/(sigma+1e-8)*sigma_ref+mu_ref, back to sRGB, clamp, cast.
//
// Two streaming kernels per transform: (1) LAB sums and sums of squares, fp64 across lanes /
// workgroups, finished by the last workgroup to arrive; (2) the fused normalise + inverse transform.
// LAB is recomputed in pass 2 instead of being stored: 24 VALU-cheap transcendentals per pixel are
// cheaper than a 12 B/px round trip through HBM.
#include "common.hpp"
#include "dispatch.hpp"
#include "tissue.hpp"
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <type_traits>

namespace sx {
namespace reinhard {

constexpr int kIters = 8;
constexpr int kSums = 6;   // per channel: sum, sum of squares (about a fixed shift)

struct alignas(256) State {
    double sums[kSums];
    float mean[3], stdv[3];      // source statistics
    unsigned int arrivals;
    // sx_reinhard_transform_ready(): no launch in front of the statistics pass that clears the arrival counters -- they are zero in a
    // READY workspace (zero-filled once, since then only touched by completed calls: the last arrivals reset them).  The statistics
    // pass leaves the call's number here and the apply pass compares: statistics that were never finished (counters that were not
    // zero) are noticed and reported through `status`.
    unsigned int stats_of_call;
    unsigned int status;         // bit 0: a *_ready call did not find the statistics of its own statistics pass
};

// Divisions by the colour-space constants are multiplications by their reciprocals (<= 1 ulp from the reference's
// divisions, far inside the 1e-4 tolerance).  fast_pow(), srgb_to_linear() and the LinearTable of uint8 pixels live in tissue.hpp:
// the tissue rule of the masked forms is written there, once, on the same linear-light values.

// 8-bit CODES of float32 tiles (round 4; the Macenko transform's Coded<F>, macenko.hip): a float tile made from a decoded image holds
// float(k) / 255 for a grey level k in every element.  The statistics pass checks that for every element -- table entry k holds the
// bits of float(k) / 255 and its linear-light value -- and leaves the tile as bytes behind the workspace; the apply pass reads a tile
// that passed as those bytes (a quarter of the input bytes; the table instead of a logarithm and an exponential per channel) and a
// tile that did not as floats.  The table holds the very expression of srgb_to_linear(): every pixel gets the bits it got before.
constexpr int kCodeCopies = 4;      // bank-striped copies of the statistics pass's table (a lane reads copy lane % 4)
struct CodeLinTable {
    uint2 e[256 * kCodeCopies];     // {bits of float(k) / 255, bits of its linear-light value}
    __device__ __forceinline__ void fill() {
        for (int t = threadIdx.x; t < 256; t += blockDim.x) {
            const float v = div255_of_level((float)t);
            const uint2 entry = make_uint2(__float_as_uint(v), __float_as_uint(srgb_to_linear(v)));
#pragma unroll
            for (int c = 0; c < kCodeCopies; ++c) e[t * kCodeCopies + c] = entry;
        }
        __syncthreads();
    }
};
struct UnitLinearTable {            // the apply pass's table for coded float tiles: linear light of float(k) / 255
    float lin[256];
    __device__ __forceinline__ void fill() {
        for (int t = threadIdx.x; t < 256; t += blockDim.x) lin[t] = srgb_to_linear(div255_of_level((float)t));
        __syncthreads();
    }
};
struct Codes {                      // where a call keeps them (null / 0: the call runs without)
    uint8_t* planes;                // [n_tiles][3][pixels]
    unsigned int* bad;              // [n_tiles]: the number of the last call whose statistics pass found a non-grey-level element in the tile
    unsigned int epoch;             // this call's number (never 0)
};

// The two 3 x 3 colour matrices on the matrix core: a matrix-vector product per pixel is nine multiply-adds on the vector ALU, or three
// v_mfma_f32_4x4x1 on a pipe that is otherwise idle (apply pass 448 -> 366 vector instructions per four pixels, statistics 245 -> 203;
// 1-4 us per call on the boxes measured, inside their spread -- SQ counters put the vector ALU at 71 % / 58 % busy in the two passes, so
// the instruction count is not the whole story; section 5 of DESIGN.md).  The instruction multiplies, in each of 16 blocks of four lanes, a 4 x 1 column (one element per lane: lane l
// holds row l % 4)
// with a 1 x 4 row (lane l holds column l % 4) and adds the 4 x 4 product to four registers per lane (register r of lane l: row r,
// column l % 4).  With the matrix's column k spread over the four lanes of every block and the lane's OWN pixel component k as the
// row element, three of them leave (M x)_r of the lane's pixel in register r.  fp32 throughout; the white point is folded into the
// matrix (rows of the forward one, columns of the inverse), a difference of an ulp from the reference's separate division.
typedef float float4v __attribute__((ext_vector_type(4)));
struct MatrixLane {
    float col[3];      // M[lane % 4][k] for k = 0..2 (row 3 of the 4 x 4 block: zeros)
};
__device__ __forceinline__ MatrixLane matrix_lane(const float (&m)[3][3]) {
    const int r = (int)(lane_id() & 3u);
    MatrixLane out;
#pragma unroll
    for (int k = 0; k < 3; ++k) out.col[k] = r == 0 ? m[0][k] : r == 1 ? m[1][k] : r == 2 ? m[2][k] : 0.0f;
    return out;
}
// (M x) for the V pixels of a pack, column by column: the V accumulator chains are independent, so no instruction waits for the one
// before it (one pixel's three on their own are a dependent chain: the compiler pads it with s_nop)
template <int V>
__device__ __forceinline__ void matrix_times_pack(const MatrixLane& m, const float (&x)[V][3], float (&y)[V][3]) {
    float4v d[V];
#pragma unroll
    for (int i = 0; i < V; ++i) d[i] = float4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < V; ++i) d[i] = __builtin_amdgcn_mfma_f32_4x4x1f32(m.col[k], x[i][k], d[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        y[i][0] = d[i][0];
        y[i][1] = d[i][1];
        y[i][2] = d[i][2];
    }
}
// linear RGB -> XYZ / white point (torch_backend.py:32-38) and XYZ -> linear RGB with the white point folded in (:89-91)
__device__ __forceinline__ MatrixLane forward_matrix() {
    const float m[3][3] = {{0.412453f / 0.95047f, 0.357580f / 0.95047f, 0.180423f / 0.95047f},
                           {0.212671f, 0.715160f, 0.072169f},
                           {0.019334f / 1.08883f, 0.119193f / 1.08883f, 0.950227f / 1.08883f}};
    return matrix_lane(m);
}
__device__ __forceinline__ MatrixLane inverse_matrix() {
    const float m[3][3] = {{3.2404542f * 0.95047f, -1.5371385f, -0.4985314f * 1.08883f},
                           {-0.9692660f * 0.95047f, 1.8760108f, 0.0415560f * 1.08883f},
                           {0.0556434f * 0.95047f, -0.2040259f, 1.0572252f * 1.08883f}};
    return matrix_lane(m);
}

// f(t) of torch_backend.py:41-42 for the three components of X/Xn, Y, Z/Zn: everything of RGB -> LAB except the last affine step
__device__ __forceinline__ void xyz_to_f(const float xyz[3], float f[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = xyz[c] > 0.008856f ? fast_pow(xyz[c], 1.0f / 3.0f) : 7.787f * xyz[c] + 16.0f / 116.0f;
}

// LAB (scaled to 0..255 as the reference does, torch_backend.py:51-53) is AFFINE in e = (f_y, f_x - f_y, f_y - f_z):
//   L = 295.8 e0 - 40.8,   a = 500 e1 + 128,   b = 200 e2 + 128.
// Both passes work on e and carry the affine step in their per-call constants: the statistics are sums of e (mean and standard
// deviation of LAB follow exactly: mean = S m_e + O, std = |S| std_e), and the normalisation (lab - mu) / sd * rs + rm followed by
// LAB -> f' collapses to one multiply-add per channel on e.  16 vector instructions per pixel less in the apply pass, 7 in the
// statistics pass; the rounding differs from the step-by-step form in the last bits (max error against the oracle unchanged).
__device__ __forceinline__ constexpr float lab_scale(int c) { return c == 0 ? 116.0f * 2.55f : c == 1 ? 500.0f : 200.0f; }
__device__ __forceinline__ constexpr float lab_offset(int c) { return c == 0 ? -16.0f * 2.55f : 128.0f; }
__device__ __forceinline__ void f_to_e(const float f[3], float e[3]) {
    e[0] = f[1];
    e[1] = f[0] - f[1];
    e[2] = f[1] - f[2];
}

// e (see above) of the V pixels of the loaded packs: the linear-light values through the table for uint8 (u holds grey levels), through
// the formula otherwise (unit values); then the matrix for the whole pack, then f and e
template <int V>
__device__ __forceinline__ void lin_to_e(const float (&lin)[V][3], const MatrixLane& fwd, float (&e)[V][3]) {
    float xyz[V][3];
    matrix_times_pack<V>(fwd, lin, xyz);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float f[3];
        xyz_to_f(xyz[i], f);
        f_to_e(f, e[i]);
    }
}
template <typename T, int V>
__device__ __forceinline__ void pack_to_lin(const float (&u)[3][V], const LinearTable* table, float (&lin)[V][3]) {
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (sizeof(T) == 1) lin[i][c] = table->lin[(int)u[c][i]]; else lin[i][c] = srgb_to_linear(u[c][i]);
        }
}
template <typename T, int V>
__device__ __forceinline__ void pack_to_e(const float (&u)[3][V], const LinearTable* table, const MatrixLane& fwd, float (&e)[V][3]) {
    float lin[V][3];
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (sizeof(T) == 1) lin[i][c] = table->lin[(int)u[c][i]]; else lin[i][c] = srgb_to_linear(u[c][i]);
        }
    lin_to_e<V>(lin, fwd, e);
}
// The masked forms: which of the pack's V pixels are tissue (bit i: pixel i) -- the caller's mask bytes (one 32-bit word for a pack of
// four) or the rule on the pack's linear-light values.  Uniform branch: a call has a mask or it has none.
template <int V>
__device__ __forceinline__ uint32_t tissue_bits(const tissue::Source& tis, int64_t pixel_index, const float (&lin)[V][3]) {
    uint32_t in = 0u;
    if (tis.mask) {
        if constexpr (V == 4) {
            const uint32_t word = *reinterpret_cast<const uint32_t*>(tis.mask + pixel_index);
#pragma unroll
            for (int i = 0; i < V; ++i) in |= ((word >> (8 * i)) & 0xFFu) ? (1u << i) : 0u;
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) in |= tis.mask[pixel_index + i] ? (1u << i) : 0u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) in |= tissue::is_tissue(lin[i][0], lin[i][1], lin[i][2], tis.y_cut) ? (1u << i) : 0u;
    }
    return in;
}
// the statistics pass of a coded call: the pack's linear-light values from the code table where every element of the wave's packs is a
// grey level, by the expression (and the tile marked) where not; the codes to the tile's planes
template <int V>
__device__ __forceinline__ void pack_to_e_coding(const float (&u)[3][V], const CodeLinTable& ct, const Codes& codes, int64_t tile, int64_t pixels, int64_t p, const MatrixLane& fwd, float (&e)[V][3]) {
    static_assert(V == 4, "a pack of four codes is one 32-bit word of a plane");
    float lin[V][3];
    uint32_t word[3], differ = 0u;
    const int copy = (int)(threadIdx.x % kCodeCopies);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        word[c] = 0u;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float x = u[c][i];
            const uint32_t k = __float_as_uint(fmaf(x, 255.0f, 8388608.0f)) & 0xFFu;      // nearest grey level (anything else fails the comparison)
            const uint2 entry = ct.e[k * kCodeCopies + copy];
            differ |= entry.x ^ __float_as_uint(x);
            lin[i][c] = __uint_as_float(entry.y);
            word[c] |= k << (8 * i);
        }
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(differ != 0u) != 0ull, 0)) {
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = u[c][i];
                asm volatile("" : "+v"(x));      // (a real branch, see macenko.hip code_pack())
                lin[i][c] = srgb_to_linear(x);
            }
        if (differ != 0u) codes.bad[tile] = codes.epoch;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(codes.planes + ((size_t)tile * 3 + c) * pixels + p) = word[c];
    lin_to_e<V>(lin, fwd, e);
}
// (uint8: the packs are loaded as grey levels, not unit values)
template <typename T, int V>
__device__ __forceinline__ void load_for_lab(const T* __restrict__ p, float (&out)[V]) {
    if constexpr (sizeof(T) == 1) load_raw<T, V>(p, out); else load_unit<T, V>(p, out);
}
// the same for the apply pass, the call's last reader of the input: non-temporal packs (common.hpp: load_pack_stream)
template <typename T, int V>
__device__ __forceinline__ void load_for_lab_last(const T* __restrict__ p, float (&out)[V]) {
    if constexpr (V == 1) {
        load_for_lab<T, V>(p, out);
    } else {
        const Pack<T, V> pk = load_pack_stream<T, V>(p);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if constexpr (sizeof(T) == 1) out[i] = raw_value<T>(pk.v[i]); else out[i] = Elem<T>::load(pk.v[i]);
        }
    }
}

__device__ __forceinline__ float f_inv(float t) { return t > 0.2068966f ? t * t * t : (t - 16.0f / 116.0f) * (1.0f / 7.787f); }   // :78-80

// linear RGB -> sRGB, clamped (:93-96)
__device__ __forceinline__ void linear_to_rgb(const float lin[3], float rgb[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = lin[c] > 0.0031308f ? 1.055f * fast_pow(lin[c], 1.0f / 2.4f) - 0.055f : 12.92f * lin[c];
        rgb[c] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
}

constexpr int kTileCounterStride = 32;      // uint32 words between two tiles' arrival counters (128 bytes: a line each)

struct Geometry {
    int64_t n_tiles, pixels;
    int blocks_per_tile, chunk;
};

// kPerTile: every tile is finished by ITS last arrival -- the same fixed-order reduction over the tile's own partial sums -- and its mean
// and standard deviation go to row `tile` of mean_out / std_out (N x 3 each, required); the State is not touched.
// kMasked (the tissue forms): sums over tissue pixels only and the exact tissue count as a seventh partial; the finishing workgroup divides
// by the count (fewer than two tissue pixels: mean and standard deviation NaN), writes it to counts_out and -- pooled form -- leaves
// the one row in mean_out / std_out without touching the State's statistics.  Same grid, same reduction order: with every pixel
// tissue the sums, and so the statistics, have the unmasked form's bits.
// (the masked form's two arguments; the unmasked instantiations take an empty struct and compile as before)
template <bool kMasked> struct MaskArgs {};
template <> struct MaskArgs<true> {
    tissue::Source tis;
    unsigned long long* counts_out;      // [N] or [1]; may be null
};
template <typename T, int V, bool kPerTile = false, bool kMasked = false>
__global__ __launch_bounds__(kStreamThreads) void stats_kernel(const T* __restrict__ images, Geometry g, State* __restrict__ st, double* __restrict__ partial, unsigned int* __restrict__ tile_arrivals, float* __restrict__ mean_out, float* __restrict__ std_out, double* __restrict__ sums_out, unsigned int call, Codes codes = Codes{nullptr, nullptr, 0u}, MaskArgs<kMasked> masked = MaskArgs<kMasked>{}) {
    constexpr int kSums = kMasked ? reinhard::kSums + 1 : reinhard::kSums;
    const int64_t tile = blockIdx.x / g.blocks_per_tile;
    const int chunk_id = blockIdx.x % g.blocks_per_tile;
    const int64_t p_begin = (int64_t)chunk_id * g.chunk, p_end = min(p_begin + g.chunk, g.pixels);
    const T* img = images + tile * 3 * g.pixels;
    __shared__ LinearTable table;
    if constexpr (sizeof(T) == 1) table.fill();
    constexpr bool kCodable = std::is_same<T, float>::value && V == 4 && !kMasked;      // (the masked forms run without the codes)
    __shared__ CodeLinTable code_table;
    const bool coding = kCodable && codes.epoch != 0u;      // (uniform over the launch)
    if constexpr (kCodable) {
        if (coding) code_table.fill();
    }
    const MatrixLane fwd = forward_matrix();
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    // (requesting the next trip's packs before working on this trip's changes nothing: 55.1 against 55.5 us)
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        float u[3][V];
#pragma unroll
        for (int c = 0; c < 3; ++c) load_for_lab<T, V>(img + c * g.pixels + p, u[c]);
        float s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
        float e[V][3];
        if constexpr (kMasked) {
            float lin[V][3];
            pack_to_lin<T, V>(u, &table, lin);
            const uint32_t in = tissue_bits<V>(masked.tis, tile * g.pixels + p, lin);
            lin_to_e<V>(lin, fwd, e);
#pragma unroll
            for (int i = 0; i < V; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) e[i][c] = (in >> i) & 1u ? e[i][c] : 0.0f;      // (+ 0 and fma(0, 0, q) are exact: background adds nothing)
            acc[6] += (double)__builtin_popcount(in);
        } else if constexpr (kCodable) {
            if (coding) pack_to_e_coding<V>(u, code_table, codes, tile, g.pixels, p, fwd, e); else pack_to_e<T, V>(u, &table, fwd, e);
        } else {
            pack_to_e<T, V>(u, &table, fwd, e);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s[c] += e[i][c];
                q[c] = fmaf(e[i][c], e[i][c], q[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[c] += (double)s[c];
            acc[3 + c] += (double)q[c];
        }
    }
    __shared__ double red[kStreamThreads / kWave][kSums];
    __shared__ bool last;
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane_id() == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        double s = 0.0;
        for (int w = 0; w < kStreamThreads / kWave; ++w) s += red[w][threadIdx.x];
        // write-through (sc1) store: visible to the finishing workgroup on any XCD once its counter add lands
        __hip_atomic_store(&partial[(int64_t)blockIdx.x * kSums + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // two levels of arrival counters: a tile's work items on the tile's own word (its own 128-byte line), the tile's last arrival
        // on the call's word.  The work items all finish within a few microseconds of each other and one address takes ~90 atomic
        // operations per microsecond: 2048 tickets from ONE word kept the last workgroups waiting for theirs
        unsigned int* mine = tile_arrivals + tile * kTileCounterStride;
        last = false;
        if (__hip_atomic_fetch_add(mine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)g.blocks_per_tile - 1) {
            __hip_atomic_store(mine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next call on this workspace
            // (one tile: its last arrival is the call's -- a fit on a reference tile is launch-bound, every dependent round trip shows)
            if constexpr (kPerTile) last = true;
            else last = g.n_tiles == 1 || __hip_atomic_fetch_add(&st->arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)g.n_tiles - 1;
        }
    }
    __syncthreads();
    if (!last) return;
    // last workgroup (of the call, or of its tile): every thread sums the partials of the workgroups b = t, t+256, ... (in that order), then a
    // fixed reduction tree joins the threads -- deterministic for a given grid, and the loads run in parallel instead of
    // one dependent chain over all workgroups
    const unsigned b_first = kPerTile ? (unsigned)(tile * g.blocks_per_tile) : 0u, b_end = kPerTile ? b_first + (unsigned)g.blocks_per_tile : gridDim.x;
    {
        double mine[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) mine[k] = 0.0;
        for (unsigned b = b_first + threadIdx.x; b < b_end; b += kStreamThreads) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) mine[k] += __hip_atomic_load(&partial[(int64_t)b * kSums + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
            const double w = wave_sum(mine[k]);
            if (lane_id() == 0) red[wave][k] = w;
        }
        __syncthreads();
        double total = 0.0;
        if (threadIdx.x < kSums)
            for (int w = 0; w < kStreamThreads / kWave; ++w) total += red[w][threadIdx.x];
        __syncthreads();
        if (threadIdx.x < kSums) {
            red[0][threadIdx.x] = total;
            if (sums_out) sums_out[threadIdx.x] = total;     // raw sums of e for a cross-rank all-reduce
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const double n = kMasked ? red[0][kSums - 1] : kPerTile ? (double)g.pixels : (double)g.n_tiles * (double)g.pixels;
        const double m = red[0][c] / n;
        const double var = n > 1.0 ? (red[0][3 + c] - red[0][c] * m) / (n - 1.0) : __longlong_as_double(0x7ff8000000000000ll);   // torch.std of one value is nan
        float mean = (float)((double)lab_scale(c) * m + (double)lab_offset(c)), sd = (float)((double)lab_scale(c) * sqrt((kPerTile || kMasked) && !(n > 1.0) ? var : fmax(var, 0.0)));      // (per tile: the nan of a one-pixel tile is kept)
        if constexpr (kMasked) {
            if (!(n > 1.0)) mean = sd;      // fewer than two tissue pixels: no statistics (every apply pass copies such a tile through)
            const int64_t row = kPerTile ? tile : 0;
            mean_out[row * 3 + c] = mean;
            std_out[row * 3 + c] = sd;
            if (c == 0 && masked.counts_out) masked.counts_out[row] = (unsigned long long)n;
        } else if constexpr (kPerTile) {
            mean_out[tile * 3 + c] = mean;
            std_out[tile * 3 + c] = sd;
        } else {
            st->mean[c] = mean;
            st->stdv[c] = sd;
            if (mean_out) {
                mean_out[c] = mean;
                std_out[c] = sd;
            }
        }
    }
    if constexpr (!kPerTile) {
        if (threadIdx.x == 0) {
            st->arrivals = 0;   // ready for the next call on this workspace
            if constexpr (!kMasked) st->stats_of_call = call;
        }
    }
}

// One work item of the apply pass: the chunk blockIdx.x names, normalised with the float32 source statistics src_mean / src_std (three
// floats each).  The pooled pass reads them from the State, the per-tile and given-statistics passes from the tile's row: one body, so
// equal statistics give equal bits whichever entry point they came through.
// (`before_statistics` runs where the pooled pass checks its workspace: behind the index arithmetic, in front of the first read of the statistics)
// kMasked (the tissue forms): a tissue pixel gets exactly the value above, a background pixel the bits of the input element; a row of
// statistics that holds a NaN (fewer than two tissue pixels) copies the whole tile through.  No seam smoothing: a hard edge.
template <typename T, int V, bool kMasked = false, class Prologue>
__device__ __forceinline__ void apply_chunk(const T* images, T* out, Geometry g, const float* src_mean, const float* src_std, const float* ref_mean, const float* ref_std, Codes codes, Prologue before_statistics, tissue::Source tis = tissue::Source{nullptr, 0.0f}) {
    const int64_t tile = blockIdx.x / g.blocks_per_tile;
    const int chunk_id = blockIdx.x % g.blocks_per_tile;
    const int64_t p_begin = (int64_t)chunk_id * g.chunk, p_end = min(p_begin + g.chunk, g.pixels);
    const T* img = images + tile * 3 * g.pixels;
    T* dst = out + tile * 3 * g.pixels;
    before_statistics();
    // lab' = (lab - mu) / (sd + 1e-8) * rs + rm per channel (:349) with lab = S e + O, then fy = (L' / 2.55 + 16) / 116,
    // fx = (a' - 128) / 500 + fy, fz = fy - (b' - 128) / 200:   f' = k e + c per channel, k = rs / (sd + 1e-8)
    float k[3], cst[3];
    bool through = false;      // (masked forms: no statistics for this tile)
    if constexpr (kMasked) {
#pragma unroll
        for (int c = 0; c < 3; ++c) through = through || !(src_std[c] == src_std[c]) || !(src_mean[c] == src_mean[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double kc = (double)ref_std[c] / ((double)src_std[c] + 1e-8);      // (one division per channel, reused for every pixel)
        const double shifted = ((double)lab_offset(c) - (double)src_mean[c]) * kc + (double)ref_mean[c];      // lab' at e = 0
        k[c] = (float)kc;
        cst[c] = (float)(c == 0 ? (shifted / 2.55 + 16.0) / 116.0 : (shifted - 128.0) / (double)lab_scale(c));
    }
    __shared__ LinearTable table;
    if constexpr (sizeof(T) == 1) table.fill();
    const MatrixLane fwd = forward_matrix(), inv = inverse_matrix();
    // a tile of grey levels (see Codes): its codes in -- four bytes per lane and plane, the linear-light values from the table -- the same float pixels out
    constexpr bool kCodable = std::is_same<T, float>::value && V == 4 && !kMasked;
    __shared__ UnitLinearTable unit_table;
    bool coded = false;
    if constexpr (kCodable) {
        coded = codes.epoch != 0u && codes.bad[tile] != codes.epoch;      // (uniform over the workgroup)
        if (coded) unit_table.fill();
    }
    const uint8_t* code_planes = kCodable && coded ? codes.planes + (size_t)tile * 3 * g.pixels : nullptr;
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
        T res[3][V];
        float e[V][3], xyz[V][3], lin[V][3];
        bool have_e = false;
        if constexpr (kCodable) {
            if (coded) {
                uint32_t word[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) word[c] = *reinterpret_cast<const uint32_t*>(code_planes + (size_t)c * g.pixels + p);
#pragma unroll
                for (int i = 0; i < V; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) lin[i][c] = unit_table.lin[(word[c] >> (8 * i)) & 0xFFu];
                lin_to_e<V>(lin, fwd, e);
                have_e = true;
            }
        }
        Pack<T, V> kept[kMasked ? 3 : 1];      // (masked forms: the input elements as they are, for the background)
        uint32_t in = 0u;
        if constexpr (kMasked) {
            float u[3][V];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (V == 1) kept[c].v[0] = img[c * g.pixels + p]; else kept[c] = load_pack_stream<T, V>(img + c * g.pixels + p);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if constexpr (sizeof(T) == 1) u[c][i] = raw_value<T>(kept[c].v[i]); else u[c][i] = Elem<T>::load(kept[c].v[i]);
                }
            }
            pack_to_lin<T, V>(u, &table, lin);
            in = through ? 0u : tissue_bits<V>(tis, tile * g.pixels + p, lin);
            lin_to_e<V>(lin, fwd, e);
        } else if (!have_e) {
            float u[3][V];
#pragma unroll
            for (int c = 0; c < 3; ++c) load_for_lab_last<T, V>(img + c * g.pixels + p, u[c]);
            pack_to_e<T, V>(u, &table, fwd, e);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            // (fy = (L / 2.55 + 16) / 116, fx = (a - 128) / 500 + fy, fz = fy - (b - 128) / 200, :70-72: folded into k and cst)
            const float fy = fmaf(k[0], e[i][0], cst[0]);
            const float fx = fmaf(k[1], e[i][1], fy + cst[1]), fz = fy - fmaf(k[2], e[i][2], cst[2]);
            xyz[i][0] = f_inv(fx);
            xyz[i][1] = f_inv(fy);
            xyz[i][2] = f_inv(fz);
        }
        matrix_times_pack<V>(inv, xyz, lin);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float back[3];
            linear_to_rgb(lin[i], back);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (sizeof(T) == 1)
                    res[c][i] = Elem<T>::store(fminf(fmaxf(back[c] * 255.0f, 0.0f), 255.0f));   // :125, :131
                else
                    res[c][i] = Elem<T>::store(back[c]);
                if constexpr (kMasked) {
                    if (!((in >> i) & 1u)) res[c][i] = kept[c].v[i];
                }
            }
        }
        // (non-temporal: the output is not read again by this library and leaves no dirty lines for the next reader to wait on --
        // the same change took 10 us off the Macenko transform)
#pragma unroll
        for (int c = 0; c < 3; ++c) store_pack_stream<T, V>(dst + c * g.pixels + p, res[c]);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void apply_kernel(const T* __restrict__ images, T* __restrict__ out, Geometry g, State* __restrict__ st, const float* __restrict__ ref_mean, const float* __restrict__ ref_std, unsigned int call, Codes codes = Codes{nullptr, nullptr, 0u}) {
    apply_chunk<T, V>(images, out, g, st->mean, st->stdv, ref_mean, ref_std, codes, [&] {
        if (call != 0 && blockIdx.x == 0 && threadIdx.x == 0 && st->stats_of_call != call) atomicOr(&st->status, 1u);      // (see State)
    });
}

// The apply pass with source statistics from device arrays: row 0 for every tile (per_tile == 0) or row `tile` (per_tile == 1)
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void apply_stats_kernel(const T* __restrict__ images, T* __restrict__ out, Geometry g, const float* __restrict__ src_mean, const float* __restrict__ src_std, int per_tile, const float* __restrict__ ref_mean, const float* __restrict__ ref_std, Codes codes = Codes{nullptr, nullptr, 0u}) {
    const int64_t row = per_tile ? blockIdx.x / g.blocks_per_tile : 0;
    apply_chunk<T, V>(images, out, g, src_mean + row * 3, src_std + row * 3, ref_mean, ref_std, codes, [] {});
}

// the tissue form of the apply pass with given statistics: one launch, statistics, reference and mask read on the device
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void apply_stats_masked_kernel(const T* __restrict__ images, T* __restrict__ out, Geometry g, const float* __restrict__ src_mean, const float* __restrict__ src_std, int per_tile, const float* __restrict__ ref_mean, const float* __restrict__ ref_std, tissue::Source tis) {
    const int64_t row = per_tile ? blockIdx.x / g.blocks_per_tile : 0;
    apply_chunk<T, V, true>(images, out, g, src_mean + row * 3, src_std + row * 3, ref_mean, ref_std, Codes{nullptr, nullptr, 0u}, [] {}, tis);
}

// sx_reinhard_apply_targets / _targets_masked: a TARGET row per tile as well (per_target == 1: row `tile`, 0: row 0), and a tile any of
// whose four rows holds a NaN is copied with the bits of its input -- one workgroup-uniform branch in front of the first pixel, in the
// unmasked form too.  Every other tile runs apply_chunk as the kernels above do: with one finite target row the bits are theirs.
__device__ __forceinline__ bool rows_have_nan(const float* sm, const float* ss, const float* tm, const float* ts) {
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) bad = bad || sm[c] != sm[c] || ss[c] != ss[c] || tm[c] != tm[c] || ts[c] != ts[c];
    return bad;
}
template <typename T, int V>
__device__ __forceinline__ void copy_chunk(const T* images, T* out, Geometry g) {
    const int64_t tile = blockIdx.x / g.blocks_per_tile;
    const int chunk_id = blockIdx.x % g.blocks_per_tile;
    const int64_t p_begin = (int64_t)chunk_id * g.chunk, p_end = min(p_begin + g.chunk, g.pixels);
    const T* img = images + tile * 3 * g.pixels;
    T* dst = out + tile * 3 * g.pixels;
    for (int64_t p = p_begin + (int64_t)threadIdx.x * V; p < p_end; p += (int64_t)kStreamThreads * V) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (V == 1) {
                dst[c * g.pixels + p] = img[c * g.pixels + p];
            } else {
                const Pack<T, V> pk = load_pack_stream<T, V>(img + c * g.pixels + p);
                store_pack_stream<T, V>(dst + c * g.pixels + p, pk.v);
            }
        }
    }
}
template <typename T, int V, bool kMasked>
__global__ __launch_bounds__(kStreamThreads) void apply_targets_kernel(const T* __restrict__ images, T* __restrict__ out, Geometry g, const float* __restrict__ src_mean, const float* __restrict__ src_std, int per_tile, const float* __restrict__ tgt_mean, const float* __restrict__ tgt_std, int per_target, tissue::Source tis) {
    const int64_t tile = blockIdx.x / g.blocks_per_tile;
    const int64_t row = per_tile ? tile : 0, trow = per_target ? tile : 0;
    const float *sm = src_mean + row * 3, *ss = src_std + row * 3, *tm = tgt_mean + trow * 3, *ts = tgt_std + trow * 3;
    if (rows_have_nan(sm, ss, tm, ts)) {      // (uniform over the workgroup: the rows are the tile's)
        copy_chunk<T, V>(images, out, g);
        return;
    }
    if constexpr (kMasked) apply_chunk<T, V, true>(images, out, g, sm, ss, tm, ts, Codes{nullptr, nullptr, 0u}, [] {}, tis);
    else apply_chunk<T, V>(images, out, g, sm, ss, tm, ts, Codes{nullptr, nullptr, 0u}, [] {});
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Sweeps of a workgroup per work item: eight on a batch that fills the chip (64 tiles of 512 x 512: 2048 work items), fewer on small
// ones -- a single 512 x 512 tile is 32 work items at eight sweeps and two launches that last as long as ONE of them; at one sweep
// it is 256 (fit + transform of BASELINE configs[0]: 52 -> see DESIGN.md section 5).  A function of the batch's shape only.
static int sweeps_for(int64_t n, int64_t pixels) {
    int sweeps = kIters;
    while (sweeps > 1 && n * ((pixels + (int64_t)kStreamThreads * 4 * sweeps - 1) / ((int64_t)kStreamThreads * 4 * sweeps)) < 512) sweeps /= 2;
    return sweeps;
}
static int blocks_for(int64_t n, int64_t pixels) {
    const int64_t chunk = (int64_t)kStreamThreads * 4 * sweeps_for(n, pixels);
    return (int)((pixels + chunk - 1) / chunk);
}
// The geometry and the grid of every streaming launch over a batch: blocks_per_tile work items of `chunk` pixels per tile.
struct Launch {
    Geometry g;
    dim3 grid;
};
static Launch geometry(int64_t n, int64_t h, int64_t w) {
    const Geometry g{n, h * w, blocks_for(n, h * w), kStreamThreads * 4 * sweeps_for(n, h * w)};
    return Launch{g, dim3((unsigned)(n * g.blocks_per_tile))};
}

__global__ void init_state_kernel(State* st, unsigned int* tile_arrivals, int64_t n_tiles) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0) {
        st->arrivals = 0;
        st->status = 0;
    }
    if (i < n_tiles) tile_arrivals[i * kTileCounterStride] = 0;
}

// mean / unbiased std of LAB from (possibly all-reduced) sums of e over n pixels per channel
__global__ void finalize_kernel(const double* __restrict__ sums, double n, State* __restrict__ st) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    const double m = sums[c] / n;
    const double var = n > 1.0 ? (sums[3 + c] - sums[c] * m) / (n - 1.0) : __longlong_as_double(0x7ff8000000000000ll);
    st->mean[c] = (float)((double)lab_scale(c) * m + (double)lab_offset(c));
    st->stdv[c] = (float)((double)lab_scale(c) * sqrt(fmax(var, 0.0)));
}

static std::atomic<unsigned int> g_calls{0};      // numbers the calls (of every element type) for the ready-state check, see State
static std::atomic<unsigned int> g_code_epoch{0x2545F491u};      // numbers the coded calls (see Codes): a flag word left by another call means nothing to this one
// coded calls: float32 tiles of whole 4-pixel packs, batches of at least 2^20 pixels; the codes and the per-tile flags lie behind the workspace
static bool coded_size(bool is_float32, int64_t n, int64_t pixels) { return is_float32 && pixels % 4 == 0 && n * pixels >= (1ll << 20); }

// ---- the workspace --------------------------------------------------------------------------------------------------------------------
// ONE walk over the areas, in their order in memory: it yields the pointers of a workspace at `base` and its end (what the size queries
// and the run functions both read).  Every kind of call -- pooled, per tile, masked -- keeps the pooled layout in front (State, arrival
// counters, partial sums): a workspace left READY by one kind stays ready for another.
//
// The per-tile arrival counters lie directly behind the State, in front of the partial sums, in a region of FIXED size for batches of up to
// kReadyTiles tiles: a completed call of ANY shape then leaves every counter of every shape zero (with the counters behind the partial
// sums -- whose size follows the shape -- a call of one shape left its fp64 sums where another shape's counters lie: a READY call of that
// other shape never saw its last arrival and normalised with stale statistics).  Larger batches: the region grows with the
// batch and a READY call is treated as a plain one (the clearing launch runs).
//
// The per-tile and the masked calls put the tiles' statistics -- N x 3 means, then N x 3 standard deviations -- where the partial sums of
// the FINEST grid (one sweep per work item) would end: the pooled size follows sweeps_for() and shrinks where a larger batch takes more
// sweeps; theirs never decreases with the batch.  The masked calls hold SEVEN partial sums per work item (the seventh: the tissue
// count), so their statistics never lie in front of the per-tile calls' and their size is never the smaller one.
constexpr int64_t kReadyTiles = 4096;
enum Kind { kPooled, kTiles, kMasked };
struct Workspace {
    State* st;
    unsigned int* tile_arrivals;
    double* partial;
    float* tile_stats;            // kTiles, kMasked
    unsigned int* code_flags;     // coded (float32 batches of coded_size(); not the masked calls): Codes::bad, Codes::planes
    uint8_t* code_planes;
};
struct WorkspaceLayout {
    Workspace ws;
    size_t end;
};
static WorkspaceLayout workspace_layout(void* base, Kind kind, int64_t n_tiles, int64_t pixels, bool coded = false) {
    WorkspaceLayout l{};
    Workspace& w = l.ws;
    const uintptr_t at = reinterpret_cast<uintptr_t>(base);
    const size_t n = (size_t)n_tiles, finest = (size_t)((pixels + (int64_t)kStreamThreads * 4 - 1) / ((int64_t)kStreamThreads * 4));
    const size_t sums = kind == kPooled ? kSums * (size_t)blocks_for(n_tiles, pixels) : (kind == kMasked ? kSums + 1 : kSums) * finest;
    size_t off = 0;
    auto area = [&](auto*& field, size_t bytes) {
        field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(at + off);
        off += align_up(bytes, 256);
    };
    area(w.st, sizeof(State));
    area(w.tile_arrivals, sizeof(unsigned int) * kTileCounterStride * (size_t)std::max<int64_t>(n_tiles, kReadyTiles));
    area(w.partial, sizeof(double) * sums * n);
    if (kind != kPooled) area(w.tile_stats, sizeof(float) * 6 * n);
    if (coded) {
        area(w.code_flags, sizeof(unsigned int) * n);
        area(w.code_planes, (size_t)3 * pixels * n);
    }
    l.end = off;
    return l;
}
static size_t workspace_bytes(Kind kind, int64_t n, int64_t pixels, bool coded = false) { return workspace_layout(nullptr, kind, n, pixels, coded).end; }

// The codes of a call (see Codes) where it takes them and its workspace has room for them, none otherwise; the epoch skips 0 ("no codes").
static Codes coded_setup(const WorkspaceLayout& l, bool takes_codes, size_t ws_bytes) {
    if (!takes_codes || ws_bytes < l.end) return Codes{nullptr, nullptr, 0u};
    Codes codes{l.ws.code_planes, l.ws.code_flags, ++g_code_epoch};
    if (codes.epoch == 0u) codes.epoch = ++g_code_epoch;
    return codes;
}

// ---- the launch rules -----------------------------------------------------------------------------------------------------------------
// Packs of four pixels: tiles of whole packs, the images and (where there is one) the output at a pack's alignment, and (where there is
// one) the mask at a word's -- a pack's mask bytes are one 32-bit word.  Single pixels otherwise.
template <typename T>
static bool vector_path(const void* images, const void* out, int64_t pixels, const uint8_t* mask = nullptr) {
    const auto aligned = [](const void* p, size_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; };      // (a null pointer: no such operand)
    return pixels % 4 == 0 && aligned(images, sizeof(T) * 4) && aligned(out, sizeof(T) * 4) && aligned(mask, 4);
}
// launch(int_constant<V>{}): V = 4 or 1
template <typename L>
static void with_pack(bool vec, L&& launch) {
    with_layout<4, /*kPlanarOnly=*/true>(vec, false, [&](auto v, auto) { launch(v); return (int)SX_OK; });
}
// The calls that are ONE launch over the images with given rows: the element type, the geometry, the pack rule, then
// launch(int_constant<V>{}, const T* images, T* out, Geometry, grid) names the kernel and its own arguments.
template <typename L>
static int run_one_launch(const char* what, int dtype, const void* images, void* out, int64_t n, int64_t h, int64_t w, const uint8_t* mask, L&& launch) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const Launch l = geometry(n, h, w);
        with_pack(vector_path<T>(images, out, l.g.pixels, mask), [&](auto v) { launch(v, static_cast<const T*>(images), static_cast<T*>(out), l.g, l.grid); });
        return check_launch(what);
    });
}

template <typename T>
static int run(const void* images, void* out, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, float* mean_out, float* std_out, double* sums_out, const double* sums_in, double n_total, void* ws, size_t ws_bytes, hipStream_t stream, bool ready) {
    const Launch l = geometry(n, h, w);
    const Geometry& g = l.g;
    const bool vec = vector_path<T>(images, out, g.pixels);
    // float32 batches, statistics and apply pass in this one call: the tiles' 8-bit codes behind the workspace (see Codes)
    const bool coded = coded_size(std::is_same<T, float>::value, n, g.pixels);
    const WorkspaceLayout lay = workspace_layout(ws, kPooled, n, g.pixels, coded);
    const Workspace& a = lay.ws;
    const Codes codes = coded_setup(lay, coded && vec && out && !sums_in && !sums_out, ws_bytes);
    if (n > kReadyTiles) ready = false;      // (the counters of such a batch do not lie in the shape-independent region)
    const T* in = static_cast<const T*>(images);
    const dim3 block(kStreamThreads);
    unsigned int call = 0;
    if (sums_in) {            // statistics come from outside (all-reduced over ranks)
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, stream, sums_in, n_total, a.st);
    } else {
        call = ++g_calls;
        if (call == 0) call = ++g_calls;      // (0 means "no check" to the apply pass)
        if (!ready) hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.st, a.tile_arrivals, n);
        with_pack(vec, [&](auto v) { hipLaunchKernelGGL((stats_kernel<T, decltype(v)::value>), l.grid, block, 0, stream, in, g, a.st, a.partial, a.tile_arrivals, mean_out, std_out, sums_out, call, codes); });
    }
    if (out) with_pack(vec, [&](auto v) { hipLaunchKernelGGL((apply_kernel<T, decltype(v)::value>), l.grid, block, 0, stream, in, static_cast<T*>(out), g, a.st, ref_mean, ref_std, ready ? call : 0u, codes); });
    return check_launch("reinhard");
}

static int dispatch(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rm, const float* rs, float* mo, float* so, double* sums_out, const double* sums_in, double n_total, void* ws, size_t ws_bytes, void* stream_ptr, bool ready = false) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (const int rc = check_sizes(n, h, w)) return rc;
    if (const int rc = check_workspace(ws, ws_bytes, workspace_bytes(kPooled, n, h * w))) return rc;      // (the dtype code: with_dtype, below)
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return run<typename decltype(t)::type>(images, out, n, h, w, rm, rs, mo, so, sums_out, sums_in, n_total, ws, ws_bytes, stream, ready); });
}

// ---- per-tile statistics ------------------------------------------------------------------------------------------------------------
// statistics pass with a finish per tile; with `out` the apply pass with the tile's own row
template <typename T>
static int run_tiles(const void* images, void* out, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, float* mean_out, float* std_out, void* ws, size_t ws_bytes, hipStream_t stream) {
    const Launch l = geometry(n, h, w);
    const Geometry& g = l.g;
    const bool vec = vector_path<T>(images, out, g.pixels);
    const bool coded = coded_size(std::is_same<T, float>::value, n, g.pixels);
    const WorkspaceLayout lay = workspace_layout(ws, kTiles, n, g.pixels, coded);
    const Workspace& a = lay.ws;
    const Codes codes = coded_setup(lay, coded && vec && out, ws_bytes);
    if (!mean_out) {      // (both or neither: checked by the entry points)
        mean_out = a.tile_stats;
        std_out = mean_out + 3 * n;
    }
    const T* in = static_cast<const T*>(images);
    const dim3 block(kStreamThreads);
    hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.st, a.tile_arrivals, n);
    with_pack(vec, [&](auto v) { hipLaunchKernelGGL((stats_kernel<T, decltype(v)::value, true>), l.grid, block, 0, stream, in, g, a.st, a.partial, a.tile_arrivals, mean_out, std_out, nullptr, 0u, codes); });
    if (out) with_pack(vec, [&](auto v) { hipLaunchKernelGGL((apply_stats_kernel<T, decltype(v)::value>), l.grid, block, 0, stream, in, static_cast<T*>(out), g, mean_out, std_out, 1, ref_mean, ref_std, codes); });
    return check_launch("reinhard (per tile)");
}

static int dispatch_tiles(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rm, const float* rs, float* mo, float* so, void* ws, size_t ws_bytes, void* stream_ptr) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (const int rc = check_sizes(n, h, w)) return rc;
    if (const int rc = dtype_ok(dtype)) return rc;
    if (const int rc = check_workspace(ws, ws_bytes, workspace_bytes(kTiles, n, h * w))) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return run_tiles<typename decltype(t)::type>(images, out, n, h, w, rm, rs, mo, so, ws, ws_bytes, stream); });
}

// ---- tissue masks -----------------------------------------------------------------------------------------------------------------
// masked statistics (a finish per tile, or one for the batch), then with `out` the masked apply pass with those rows
template <typename T>
static int run_masked(const void* images, void* out, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, tissue::Source tis, bool per_tile, float* mean_out, float* std_out, unsigned long long* counts_out, void* ws, hipStream_t stream) {
    const Launch l = geometry(n, h, w);
    const Geometry& g = l.g;
    const bool vec = vector_path<T>(images, out, g.pixels, tis.mask);
    const Workspace a = workspace_layout(ws, kMasked, n, g.pixels).ws;
    if (!mean_out) {      // (both or neither: checked by the entry points)
        mean_out = a.tile_stats;
        std_out = mean_out + 3 * n;
    }
    const T* in = static_cast<const T*>(images);
    const dim3 block(kStreamThreads);
    hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.st, a.tile_arrivals, n);
    with_flags(vec, per_tile, [&](auto kVec, auto kPerTile) {
        hipLaunchKernelGGL((stats_kernel<T, decltype(kVec)::value ? 4 : 1, decltype(kPerTile)::value, true>), l.grid, block, 0, stream, in, g, a.st, a.partial, a.tile_arrivals, mean_out, std_out, nullptr, 0u, Codes{nullptr, nullptr, 0u}, MaskArgs<true>{tis, counts_out});
    });
    if (out) with_pack(vec, [&](auto v) { hipLaunchKernelGGL((apply_stats_masked_kernel<T, decltype(v)::value>), l.grid, block, 0, stream, in, static_cast<T*>(out), g, mean_out, std_out, per_tile ? 1 : 0, ref_mean, ref_std, tis); });
    return check_launch("reinhard (tissue mask)");
}

static int dispatch_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rm, const float* rs, const uint8_t* mask, double threshold, int per_tile, float* mo, float* so, unsigned long long* co, void* ws, size_t ws_bytes, void* stream_ptr) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (const int rc = check_sizes(n, h, w)) return rc;
    if (const int rc = tissue::check_source(mask, threshold)) return rc;
    if (const int rc = dtype_ok(dtype)) return rc;
    if (const int rc = check_workspace(ws, ws_bytes, workspace_bytes(kMasked, n, h * w))) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const tissue::Source tis = tissue::source_of(mask, threshold);
    return with_dtype(dtype, [&](auto t) { return run_masked<typename decltype(t)::type>(images, out, n, h, w, rm, rs, tis, per_tile != 0, mo, so, co, ws, stream); });
}

// sx_tissue_mask: the rule as a call of its own.  Workgroup b takes share b % blocks_per_tile of tile b / blocks_per_tile; a thread a pack
// of four pixels (planar tiles of whole packs at aligned addresses) or single pixels; mask bytes 1 / 0 and the tile's tissue count.
constexpr int kMaskBlocksPerTile = 64;
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void tissue_mask_kernel(const T* __restrict__ images, int64_t pixels, int channels_last, int blocks_per_tile, float y_cut, uint8_t* __restrict__ mask_out, unsigned long long* __restrict__ counts_out) {
    __shared__ LinearTable table;
    if constexpr (sizeof(T) == 1) table.fill();
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;      // element (p, c) of a tile: p * step + c * plane
    unsigned int mine = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        T v[3][V];
        if constexpr (V == 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][0] = img[p * step + c * plane];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(img + c * pixels + p);      // (planar only)
#pragma unroll
                for (int i = 0; i < V; ++i) v[c][i] = pk.v[i];
            }
        }
        uint8_t m[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            m[i] = tissue::is_tissue(tissue::linear_of<T>(v[0][i], table), tissue::linear_of<T>(v[1][i], table), tissue::linear_of<T>(v[2][i], table), y_cut) ? 1 : 0;
            mine += m[i];
        }
        if (mask_out) store_pack<uint8_t, V>(mask_out + tile * pixels + p, m);
    }
    if (counts_out) {
        __shared__ unsigned int parts[kStreamThreads / kWave];
        const unsigned int total = wave_total_u32(mine);
        if (lane_id() == 0) parts[threadIdx.x / kWave] = total;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long sum = 0;
            for (int k = 0; k < kStreamThreads / kWave; ++k) sum += parts[k];
            if (sum) atomicAdd(&counts_out[tile], sum);
        }
    }
}

template <typename T>
static int run_tissue_mask(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, float y_cut, uint8_t* mask_out, unsigned long long* counts_out, hipStream_t stream) {
    const int64_t pixels = h * w;
    if (counts_out && hipMemsetAsync(counts_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    const bool vec = !channels_last && vector_path<T>(images, nullptr, pixels, mask_out);      // (the mask written: a pack's bytes are one word, as of a mask read)
    const int per_block = kStreamThreads * (vec ? 4 : 1);
    const int blocks_per_tile = (int)std::min<int64_t>((pixels + per_block - 1) / per_block, kMaskBlocksPerTile);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    with_pack(vec, [&](auto v) { hipLaunchKernelGGL((tissue_mask_kernel<T, decltype(v)::value>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, y_cut, mask_out, counts_out); });
    return check_launch("tissue mask");
}

}  // namespace reinhard
}  // namespace sx

using namespace sx;

extern "C" size_t sx_reinhard_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return reinhard::workspace_bytes(reinhard::kPooled, n, h * w);
}
// ... with room for the 8-bit codes of a float32 batch (3 bytes per pixel): sx_reinhard_transform(_ready) then reads the tiles that consist
// of grey levels as bytes in its second pass.  A call on the smaller workspace of sx_reinhard_workspace_bytes() runs without.
extern "C" size_t sx_reinhard_workspace_bytes_for(int dtype, int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return reinhard::workspace_bytes(reinhard::kPooled, n, h * w, reinhard::coded_size(dtype == SX_F32, n, h * w));
}

extern "C" int sx_reinhard_fit(const void* images, int dtype, int64_t n, int64_t h, int64_t w, float* mean_out, float* std_out, void* ws, size_t ws_bytes, void* stream) {
    if (!mean_out || !std_out) return fail(SX_ERR_BAD_ARG, "mean_out / std_out pointer is null");
    return reinhard::dispatch(images, nullptr, dtype, n, h, w, nullptr, nullptr, mean_out, std_out, nullptr, nullptr, 0.0, ws, ws_bytes, stream);
}

extern "C" int sx_reinhard_transform(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "out / ref_mean / ref_std pointer is null");
    return reinhard::dispatch(images, out, dtype, n, h, w, ref_mean, ref_std, nullptr, nullptr, nullptr, nullptr, 0.0, ws, ws_bytes, stream);
}

// The transform on a workspace in the READY state (see State): zero-filled once by sx_reinhard_workspace_init(), since then only touched
// by completed calls of this section.  No clearing launch in front of the statistics pass (~4 us of a 130 us call).
extern "C" int sx_reinhard_workspace_init(void* ws, size_t ws_bytes, void* stream) {
    if (!ws || ws_bytes < sizeof(reinhard::State)) return fail(SX_ERR_WORKSPACE, "workspace too small: need at least %zu bytes, got %zu", sizeof(reinhard::State), ws_bytes);
    if (hipMemsetAsync(ws, 0, ws_bytes, static_cast<hipStream_t>(stream)) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    return SX_OK;
}

extern "C" size_t sx_reinhard_workspace_status_offset(void) { return offsetof(reinhard::State, status); }

extern "C" int sx_reinhard_transform_ready(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "out / ref_mean / ref_std pointer is null");
    return reinhard::dispatch(images, out, dtype, n, h, w, ref_mean, ref_std, nullptr, nullptr, nullptr, nullptr, 0.0, ws, ws_bytes, stream, true);
}

// Batch statistics pooled ACROSS RANKS: local shifted sums out, all-reduce on the host side, apply with the global sums.
extern "C" int sx_reinhard_sums(const void* images, int dtype, int64_t n, int64_t h, int64_t w, double* sums_out, void* ws, size_t ws_bytes, void* stream) {
    if (!sums_out) return fail(SX_ERR_BAD_ARG, "sums_out pointer is null");
    return reinhard::dispatch(images, nullptr, dtype, n, h, w, nullptr, nullptr, nullptr, nullptr, sums_out, nullptr, 0.0, ws, ws_bytes, stream);
}

extern "C" int sx_reinhard_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const double* sums, double n_total_pixels, const float* ref_mean, const float* ref_std, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !sums || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "out / sums / ref_mean / ref_std pointer is null");
    if (!(n_total_pixels >= 1.0)) return fail(SX_ERR_BAD_ARG, "n_total_pixels must be >= 1");
    return reinhard::dispatch(images, out, dtype, n, h, w, ref_mean, ref_std, nullptr, nullptr, nullptr, sums, n_total_pixels, ws, ws_bytes, stream);
}

// Per-tile source statistics (torchstain's, tiatoolbox's, HistomicsTK's Reinhard works on ONE image): the pooled statistics pass with a
// finish per tile, and the pooled apply pass's arithmetic on the tile's own row.
extern "C" size_t sx_reinhard_tiles_workspace_bytes(int dtype, int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return reinhard::workspace_bytes(reinhard::kTiles, n, h * w, reinhard::coded_size(dtype == SX_F32, n, h * w));
}

extern "C" int sx_reinhard_tile_stats(const void* images, int dtype, int64_t n, int64_t h, int64_t w, float* tile_mean_out, float* tile_std_out, void* ws, size_t ws_bytes, void* stream) {
    if (!tile_mean_out || !tile_std_out) return fail(SX_ERR_BAD_ARG, "tile_mean_out / tile_std_out pointer is null");
    return reinhard::dispatch_tiles(images, nullptr, dtype, n, h, w, nullptr, nullptr, tile_mean_out, tile_std_out, ws, ws_bytes, stream);
}

extern "C" int sx_reinhard_transform_tiles(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, float* tile_mean_out, float* tile_std_out, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "out / ref_mean / ref_std pointer is null");
    if ((tile_mean_out == nullptr) != (tile_std_out == nullptr)) return fail(SX_ERR_BAD_ARG, "tile_mean_out and tile_std_out: both or neither");
    return reinhard::dispatch_tiles(images, out, dtype, n, h, w, ref_mean, ref_std, tile_mean_out, tile_std_out, ws, ws_bytes, stream);
}

// the apply pass alone, with the caller's statistics: one launch (kMasked: the tissue form, below)
template <bool kMasked>
static int apply_stats_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* ref_mean, const float* ref_std, const uint8_t* mask, double luminosity_threshold, void* stream_ptr) {
    if (!images || !out) return fail(SX_ERR_BAD_ARG, "images / out pointer is null");
    if (!source_mean || !source_std || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "source_mean / source_std / ref_mean / ref_std pointer is null");
    if (const int rc = check_sizes(n, h, w)) return rc;
    if (const int rc = check_rows("n_sources", n_sources, n)) return rc;
    if constexpr (kMasked) {
        if (const int rc = tissue::check_source(mask, luminosity_threshold)) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int per_tile = rows_per_tile(n_sources, n);
    return reinhard::run_one_launch(kMasked ? "reinhard (given statistics, tissue mask)" : "reinhard (given statistics)", dtype, images, out, n, h, w, mask, [&](auto v, auto* in, auto* dst, const reinhard::Geometry& g, dim3 grid) {
        using T = std::remove_pointer_t<decltype(dst)>;
        if constexpr (kMasked)
            hipLaunchKernelGGL((reinhard::apply_stats_masked_kernel<T, decltype(v)::value>), grid, dim3(kStreamThreads), 0, stream, in, dst, g, source_mean, source_std, per_tile, ref_mean, ref_std, tissue::source_of(mask, luminosity_threshold));
        else
            hipLaunchKernelGGL((reinhard::apply_stats_kernel<T, decltype(v)::value>), grid, dim3(kStreamThreads), 0, stream, in, dst, g, source_mean, source_std, per_tile, ref_mean, ref_std, reinhard::Codes{nullptr, nullptr, 0u});
    });
}

extern "C" int sx_reinhard_apply_stats(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* ref_mean, const float* ref_std, void* stream_ptr) {
    return apply_stats_call<false>(images, out, dtype, n, h, w, source_mean, source_std, n_sources, ref_mean, ref_std, nullptr, 0.0, stream_ptr);
}

// ---- tissue masks (an extension: HistomicsTK's reinhard(mask_out=), staintools' LuminosityThresholdTissueLocator) ------------------------------
extern "C" int sx_tissue_mask(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, double luminosity_threshold, uint8_t* mask_out, unsigned long long* tile_counts_out, void* stream_ptr) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!mask_out && !tile_counts_out) return fail(SX_ERR_BAD_ARG, "mask_out and tile_counts_out are both null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (n > 0x7fffffffll / reinhard::kMaskBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    if (!tissue::threshold_ok(luminosity_threshold)) return fail(SX_ERR_BAD_ARG, "luminosity_threshold must lie in (0, 1), got %g", luminosity_threshold);
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const float y_cut = tissue::y_cut_of(luminosity_threshold);
    return with_dtype(dtype, [&](auto t) { return reinhard::run_tissue_mask<typename decltype(t)::type>(images, n, h, w, channels_last, y_cut, mask_out, tile_counts_out, stream); });
}

extern "C" size_t sx_reinhard_masked_workspace_bytes(int dtype, int64_t n, int64_t h, int64_t w) {
    (void)dtype;
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return reinhard::workspace_bytes(reinhard::kMasked, n, h * w);
}

extern "C" int sx_reinhard_stats_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const uint8_t* mask, double luminosity_threshold, int per_tile, float* mean_out, float* std_out, unsigned long long* counts_out, void* ws, size_t ws_bytes, void* stream) {
    if (!mean_out || !std_out) return fail(SX_ERR_BAD_ARG, "mean_out / std_out pointer is null");
    return reinhard::dispatch_masked(images, nullptr, dtype, n, h, w, nullptr, nullptr, mask, luminosity_threshold, per_tile, mean_out, std_out, counts_out, ws, ws_bytes, stream);
}

extern "C" int sx_reinhard_transform_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* ref_mean, const float* ref_std, const uint8_t* mask, double luminosity_threshold, int per_tile, float* mean_out, float* std_out, unsigned long long* counts_out, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_mean || !ref_std) return fail(SX_ERR_BAD_ARG, "out / ref_mean / ref_std pointer is null");
    if ((mean_out == nullptr) != (std_out == nullptr)) return fail(SX_ERR_BAD_ARG, "mean_out and std_out: both or neither");
    return reinhard::dispatch_masked(images, out, dtype, n, h, w, ref_mean, ref_std, mask, luminosity_threshold, per_tile, mean_out, std_out, counts_out, ws, ws_bytes, stream);
}

extern "C" int sx_reinhard_apply_stats_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* ref_mean, const float* ref_std, const uint8_t* mask, double luminosity_threshold, void* stream_ptr) {
    return apply_stats_call<true>(images, out, dtype, n, h, w, source_mean, source_std, n_sources, ref_mean, ref_std, mask, luminosity_threshold, stream_ptr);
}

// ---- a target per tile (statistics-space augmentation, Reinhard to per-tile / per-slide targets without a fit) ------------------------------
// the geometry and the pack rule of the two calls above, one launch
template <bool kMasked>
static int apply_targets_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* target_mean, const float* target_std, int64_t n_targets, const uint8_t* mask, double luminosity_threshold, void* stream_ptr) {
    if (!images || !out) return fail(SX_ERR_BAD_ARG, "images / out pointer is null");
    if (!source_mean || !source_std || !target_mean || !target_std) return fail(SX_ERR_BAD_ARG, "source_mean / source_std / target_mean / target_std pointer is null");
    if (const int rc = check_sizes(n, h, w)) return rc;
    if (const int rc = check_rows("n_sources", n_sources, n)) return rc;
    if (const int rc = check_rows("n_targets", n_targets, n)) return rc;
    if constexpr (kMasked) {
        if (const int rc = tissue::check_source(mask, luminosity_threshold)) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int per_tile = rows_per_tile(n_sources, n), per_target = rows_per_tile(n_targets, n);
    const tissue::Source tis = kMasked ? tissue::source_of(mask, luminosity_threshold) : tissue::Source{nullptr, 0.0f};
    return reinhard::run_one_launch(kMasked ? "reinhard (targets per tile, tissue mask)" : "reinhard (targets per tile)", dtype, images, out, n, h, w, mask, [&](auto v, auto* in, auto* dst, const reinhard::Geometry& g, dim3 grid) {
        using T = std::remove_pointer_t<decltype(dst)>;
        hipLaunchKernelGGL((reinhard::apply_targets_kernel<T, decltype(v)::value, kMasked>), grid, dim3(kStreamThreads), 0, stream, in, dst, g, source_mean, source_std, per_tile, target_mean, target_std, per_target, tis);
    });
}

extern "C" int sx_reinhard_apply_targets(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* target_mean, const float* target_std, int64_t n_targets, void* stream_ptr) {
    return apply_targets_call<false>(images, out, dtype, n, h, w, source_mean, source_std, n_sources, target_mean, target_std, n_targets, nullptr, 0.0, stream_ptr);
}

extern "C" int sx_reinhard_apply_targets_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* source_mean, const float* source_std, int64_t n_sources, const float* target_mean, const float* target_std, int64_t n_targets, const uint8_t* mask, double luminosity_threshold, void* stream_ptr) {
    return apply_targets_call<true>(images, out, dtype, n, h, w, source_mean, source_std, n_sources, target_mean, target_std, n_targets, mask, luminosity_threshold, stream_ptr);
}

// ---- tissue detection: luminosity histograms (for Otsu thresholds), per-tile cuts, binary morphology on masks ------------------------------
#include "tissue_detect.hpp"

// ---- connected components of masks, and the area filters on them ----------------------------------------------------------------------
#include "components.hpp"

// ---- saturation-channel tissue detection: saturation maps, the median filter, level histograms and level thresholds ------------------------
#include "saturation.hpp"

// ---- focus measurement: grey maps, the integer sums of the Laplacian and the Sobel gradient per tile, cell or batch, cell grids as masks -------
#include "focus.hpp"

// ---- grey statistics: pixels, sum Y and sum Y^2 per tile or batch in one launch, on focus.hpp's grey level (the pivot of tone.hpp's contrast) ----
#include "tone_statistics.hpp"

// ---- luminosity standardisation: the exact percentile of the luminance, the one-launch L* map ------------------------------------------------
#include "luminosity.hpp"
