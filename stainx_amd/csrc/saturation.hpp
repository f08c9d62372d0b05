// Saturation-channel tissue detection (included from reinhard.hip beside tissue_detect.hpp, whose grid and loads the streaming kernels
// here share): the HSV saturation of a batch as 8-bit levels, a median filter on level maps, the 256-bin histogram of a level map and
// the threshold `level > t` with t per tile in device memory.  Every result is an integer and every definition exact.
//
// The 8-bit level of a stored element: a uint8 is its own level; any other type gives rintf(fminf(fmaxf(255.0f * v, 0.0f), 255.0f)) of
// its unit value v = Elem<T>::load(x) -- one float32 multiply, a clamp, round-half-even.  The saturation of a pixel with largest level M
// and smallest m: 0 if M == 0, else (510 (M - m) + M) / (2 M) in integers, which is 255 (M - m) / M rounded half up.  A pixel with a NaN
// in any channel has saturation 0.
#pragma once

#include <algorithm>
#include <type_traits>

#include "tissue_detect.hpp"

namespace sx {
namespace saturation {

template <typename T>
__device__ __forceinline__ int level_of(T x, bool& nan) {
    if constexpr (std::is_same<T, uint8_t>::value) {
        return (int)x;
    } else {
        const float v = Elem<T>::load(x);
        nan = nan || v != v;
        return (int)rintf(fminf(fmaxf(255.0f * v, 0.0f), 255.0f));
    }
}

template <typename T>
__device__ __forceinline__ uint8_t saturation_of(T r, T g, T b) {
    bool nan = false;
    const int lr = level_of<T>(r, nan), lg = level_of<T>(g, nan), lb = level_of<T>(b, nan);
    const int hi = max(lr, max(lg, lb)), lo = min(lr, min(lg, lb));
    if (nan || hi == 0) return 0;
    return (uint8_t)((uint32_t)(510 * (hi - lo) + hi) / (uint32_t)(2 * hi));
}

// The grid, loads and layouts of detect::tissue_mask_tiles_kernel.
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void saturation_map_kernel(const T* __restrict__ images, int64_t pixels, int channels_last, int blocks_per_tile, uint8_t* __restrict__ out) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        T v[3][V];
        detect::load_pixels<T, V>(img, p, pixels, step, plane, v);
        uint8_t s[V];
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = saturation_of<T>(v[0][i], v[1][i], v[2][i]);
        store_pack<uint8_t, V>(out + tile * pixels + p, s);
    }
}

template <typename T>
static int run_saturation_map(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, uint8_t* out, hipStream_t stream) {
    const int64_t pixels = h * w;
    const bool vec = !channels_last && pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const int per_block = kStreamThreads * (vec ? 4 : 1);
    const int blocks_per_tile = (int)std::min<int64_t>((pixels + per_block - 1) / per_block, detect::kBlocksPerTile);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((saturation_map_kernel<T, 4>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, out);
    else
        hipLaunchKernelGGL((saturation_map_kernel<T, 1>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, out);
    return check_launch("saturation map");
}

// ---- the histogram of a level map: the scheme of detect::luminosity_histogram_kernel (a copy of the histogram per bank, runs of equal
// levels counted by the lane and added once) with the level itself as the bin.
template <int V>
__global__ __launch_bounds__(kStreamThreads) void level_histogram_kernel(const uint8_t* __restrict__ levels, int64_t pixels, int blocks_per_tile, int pooled, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t hist[detect::kHistBins][detect::kHistCopies];
    for (int i = threadIdx.x; i < detect::kHistBins * detect::kHistCopies; i += kStreamThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const uint8_t* src = levels + tile * pixels;
    uint32_t* mine = &hist[0][threadIdx.x & (detect::kHistCopies - 1)];
    uint32_t last = 0, run = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        uint8_t v[V];
        if constexpr (V == 1) {
            v[0] = src[p];
        } else {
            const Pack<uint8_t, V> pk = *reinterpret_cast<const Pack<uint8_t, V>*>(src + p);
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = pk.v[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint32_t b = v[i];
            if (b == last) {
                ++run;
            } else {
                if (run) atomicAdd(&mine[last * detect::kHistCopies], run);
                last = b;
                run = 1;
            }
        }
    }
    if (run) atomicAdd(&mine[last * detect::kHistCopies], run);
    __syncthreads();
    for (int t = threadIdx.x; t < detect::kHistBins; t += kStreamThreads) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < detect::kHistCopies; ++k) sum += hist[t][(t + k) & (detect::kHistCopies - 1)];
        if (sum) atomicAdd(&counts[(pooled ? 0 : tile) * detect::kHistBins + t], sum);
    }
}

// ---- level > threshold of the tile, the threshold read from device memory; counts by wave sums as detect::tissue_mask_tiles_kernel
template <int V>
__global__ __launch_bounds__(kStreamThreads) void level_mask_tiles_kernel(const uint8_t* __restrict__ levels, int64_t pixels, int blocks_per_tile, const int32_t* __restrict__ tile_thresholds, uint8_t* __restrict__ mask_out, unsigned long long* __restrict__ counts_out) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const int threshold = tile_thresholds[tile];
    const uint8_t* src = levels + tile * pixels;
    unsigned int mine = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        uint8_t v[V], m[V];
        if constexpr (V == 1) {
            v[0] = src[p];
        } else {
            const Pack<uint8_t, V> pk = *reinterpret_cast<const Pack<uint8_t, V>*>(src + p);
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = pk.v[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            m[i] = (int)v[i] > threshold ? 1 : 0;
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

static int level_blocks_per_tile(int64_t pixels, bool vec) {
    const int per_block = kStreamThreads * (vec ? 4 : 1);
    return (int)std::min<int64_t>((pixels + per_block - 1) / per_block, detect::kBlocksPerTile);
}

// ---- the median filter -----------------------------------------------------------------------------------------------------------------
// A workgroup writes kMedianRows x kMedianCols levels of one tile.  It stages them with a halo ON CHIP ONCE -- as BIT PLANES: a wave
// takes a staged row, a lane a column, and __ballot packs bit b of the 64 levels into a word pair, for b = 0..7 (the staging of
// detect::morphology_kernel, eight times).  A staged row holds the 32 columns left of the block, the block's 64 and the 32 to its
// right as four 32-column words of eight planes each.  Every coordinate is clamped to the tile as it is staged: the replicated border
// costs nothing later, no load leaves the tile and tiles never see each other.
//
// Then a wave takes an output row and a lane a column.  The K levels of a window row are K consecutive bits of each plane: the lane
// reads the two words they may span for all eight planes as one run of 64 bytes and brings the window's first column to bit 0 with one
// v_alignbit per plane.  The lanes of a read touch two or three such runs, 32 bytes apart: broadcasts, no bank conflict.
//
// The value of rank (K^2 + 1) / 2 is found by a radix selection over the 8 bits, a WINDOW ROW per operation: cand[r] holds a bit for
// every level of row r that still matches the bits chosen so far (at first the low K bits), `above` counts the levels already known to
// be larger.  For bit b, above + sum over r of popcount(x[r][b] & cand[r]) is the number of window levels >= prefix | bit; the bit is
// kept iff that reaches the rank (K^2 is odd: the rank from below is the rank from above), otherwise `above` takes the count; then
// cand[r] &= x[r][b] ^ flip keeps the candidates whose bit b agrees with the choice.  An alignbit, an AND and a v_bcnt (which adds) to
// count, an XNOR and an AND to narrow: 5 operations per window ROW and bit -- 40 K per output pixel, where the compare-and-count of single
// levels takes 16 K^2.  The window size is a compile-time parameter: the loops unroll and the window's planes live in registers.
constexpr int kMedianRows = 64;
constexpr int kMedianCols = 64;
constexpr int kMedianThreads = 256;
constexpr int kMedianMaxSize = SX_MEDIAN_MAX_SIZE;
constexpr int kMedianSide = 32;         // staged columns either side of the block: one 32-column word
constexpr int kMedianWords = (kMedianCols + 2 * kMedianSide) / 32;
static_assert(kMedianCols == kWave && kMedianThreads % kWave == 0, "a wave takes a row, a lane a column; a ballot is 64 columns");
static_assert(kMedianMaxSize / 2 <= kMedianSide && kMedianMaxSize <= 32, "a window row lies inside the staged row and inside the 32 bits an alignbit gives");

template <int K>
__global__ __launch_bounds__(kMedianThreads) void median_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t height, int64_t width, int row_blocks, int col_blocks) {
    constexpr int kHalf = K / 2, kRank = (K * K + 1) / 2, kWaves = kMedianThreads / kWave;
    __shared__ __attribute__((aligned(16))) uint32_t planes[kMedianRows + 2 * kHalf][kMedianWords][8];
    const int per_tile = row_blocks * col_blocks;
    const int64_t tile = blockIdx.x / per_tile;
    const int within = blockIdx.x % per_tile;
    const int64_t y0 = (int64_t)(within / col_blocks) * kMedianRows, x0 = (int64_t)(within % col_blocks) * kMedianCols;
    const uint8_t* src = in + tile * height * width;
    uint8_t* dst = out + tile * height * width;
    const int rows_out = (int)min((int64_t)kMedianRows, height - y0);
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (int row = wave; row < rows_out + 2 * kHalf; row += kWaves) {      // (uniform in a wave: every lane votes)
        const int64_t gy = min(max(y0 - kHalf + row, (int64_t)0), height - 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int64_t gx = min(max(x0 - kMedianSide + half * kWave + lane, (int64_t)0), width - 1);
            const uint32_t level = src[gy * width + gx];
            uint32_t mine = 0;      // lanes 0..7 keep planes 0..7 of the low word, lanes 8..15 of the high word
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t bits = __ballot((level >> b) & 1u);
                if ((lane & 7) == b) mine = (lane & 8) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
            }
            if (lane < 16) planes[row][2 * half + (lane >> 3)][lane & 7] = mine;
        }
    }
    __syncthreads();
    if (x0 + lane >= width) return;      // (after the only barrier, and after the last vote)
    const int first = kMedianSide + lane - kHalf;      // the staged column of the window's left edge: 25..95
    const int word = first >> 5;                       // 0..2: the window lies in words word and word + 1
    const uint32_t shift = (uint32_t)(first & 31);
    for (int oy = wave; oy < rows_out; oy += kWaves) {
        uint32_t x[K][8], cand[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const uint32_t* lo = &planes[oy + r][word][0];
#pragma unroll
            for (int b = 0; b < 8; ++b) x[r][b] = __builtin_amdgcn_alignbit(lo[8 + b], lo[b], shift);
            cand[r] = (1u << K) - 1u;
        }
        uint32_t prefix = 0, above = 0;
#pragma unroll
        for (int b = 7; b >= 0; --b) {
            uint32_t count = above;
#pragma unroll
            for (int r = 0; r < K; ++r) count += (uint32_t)__popc(x[r][b] & cand[r]);
            const bool keep = count >= (uint32_t)kRank;
            const uint32_t flip = keep ? 0u : ~0u;      // candidates go on with bit b set (kept) or clear
            if (keep) prefix |= 1u << b; else above = count;
#pragma unroll
            for (int r = 0; r < K; ++r) cand[r] &= x[r][b] ^ flip;
        }
        dst[(y0 + oy) * width + x0 + lane] = (uint8_t)prefix;
    }
}

static bool median_grid(int64_t n, int64_t h, int64_t w, int* row_blocks, int* col_blocks, unsigned* grid) {
    const int64_t rb = (h + kMedianRows - 1) / kMedianRows, cb = (w + kMedianCols - 1) / kMedianCols;
    if (rb > 0x7fffffffll || cb > 0x7fffffffll || rb * cb > 0x7fffffffll || n > 0x7fffffffll / (rb * cb)) return false;
    *row_blocks = (int)rb;
    *col_blocks = (int)cb;
    *grid = (unsigned)(n * rb * cb);
    return true;
}

template <int K>
static void launch_median(const uint8_t* in, uint8_t* out, int64_t h, int64_t w, int row_blocks, int col_blocks, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL((median_kernel<K>), dim3(grid), dim3(kMedianThreads), 0, stream, in, out, h, w, row_blocks, col_blocks);
}

}  // namespace saturation
}  // namespace sx

extern "C" int sx_saturation_map(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, uint8_t* levels_out, void* stream_ptr) {
    using namespace sx;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!levels_out) return fail(SX_ERR_BAD_ARG, "levels_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return saturation::run_saturation_map<typename decltype(t)::type>(images, n, h, w, channels_last, levels_out, stream); });
}

extern "C" int sx_median_filter_u8(const uint8_t* levels_in, uint8_t* levels_out, int64_t n, int64_t h, int64_t w, int size, void* stream_ptr) {
    using namespace sx;
    if (!levels_in || !levels_out) return fail(SX_ERR_BAD_ARG, "levels_in / levels_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "level maps must have positive sizes");
    if (size < 3 || size > SX_MEDIAN_MAX_SIZE || size % 2 == 0) return fail(SX_ERR_BAD_ARG, "size must be odd and lie in 3..%d, got %d", SX_MEDIAN_MAX_SIZE, size);
    if (levels_out == levels_in) return fail(SX_ERR_BAD_ARG, "levels_out must not be levels_in: the filter is not in place");
    int row_blocks = 0, col_blocks = 0;
    unsigned grid = 0;
    if (!saturation::median_grid(n, h, w, &row_blocks, &col_blocks, &grid)) return fail(SX_ERR_BAD_ARG, "level maps too large for one call");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    switch (size) {
        case 3: saturation::launch_median<3>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        case 5: saturation::launch_median<5>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        case 7: saturation::launch_median<7>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        case 9: saturation::launch_median<9>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        case 11: saturation::launch_median<11>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        case 13: saturation::launch_median<13>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
        default: saturation::launch_median<15>(levels_in, levels_out, h, w, row_blocks, col_blocks, grid, stream); break;
    }
    return check_launch("median filter");
}

extern "C" int sx_level_histogram(const uint8_t* levels, int64_t n, int64_t h, int64_t w, int pooled, unsigned long long* counts_out, void* stream_ptr) {
    using namespace sx;
    if (!levels) return fail(SX_ERR_BAD_ARG, "levels pointer is null");
    if (!counts_out) return fail(SX_ERR_BAD_ARG, "counts_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "level maps must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int64_t pixels = h * w;
    if (hipMemsetAsync(counts_out, 0, sizeof(unsigned long long) * detect::kHistBins * (size_t)(pooled ? 1 : n), stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    const bool vec = pixels % 4 == 0 && reinterpret_cast<uintptr_t>(levels) % 4 == 0;
    const int blocks_per_tile = saturation::level_blocks_per_tile(pixels, vec);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((saturation::level_histogram_kernel<4>), dim3(grid), dim3(kStreamThreads), 0, stream, levels, pixels, blocks_per_tile, pooled != 0, counts_out);
    else
        hipLaunchKernelGGL((saturation::level_histogram_kernel<1>), dim3(grid), dim3(kStreamThreads), 0, stream, levels, pixels, blocks_per_tile, pooled != 0, counts_out);
    return check_launch("level histogram");
}

extern "C" int sx_level_mask_tiles(const uint8_t* levels, int64_t n, int64_t h, int64_t w, const int32_t* tile_thresholds, uint8_t* mask_out, unsigned long long* tile_counts_out, void* stream_ptr) {
    using namespace sx;
    if (!levels) return fail(SX_ERR_BAD_ARG, "levels pointer is null");
    if (!mask_out && !tile_counts_out) return fail(SX_ERR_BAD_ARG, "mask_out and tile_counts_out are both null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "level maps must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    if (!tile_thresholds) return fail(SX_ERR_BAD_ARG, "tile_thresholds pointer is null");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int64_t pixels = h * w;
    if (tile_counts_out && hipMemsetAsync(tile_counts_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    const bool vec = pixels % 4 == 0 && reinterpret_cast<uintptr_t>(levels) % 4 == 0 && reinterpret_cast<uintptr_t>(mask_out) % 4 == 0;
    const int blocks_per_tile = saturation::level_blocks_per_tile(pixels, vec);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((saturation::level_mask_tiles_kernel<4>), dim3(grid), dim3(kStreamThreads), 0, stream, levels, pixels, blocks_per_tile, tile_thresholds, mask_out, tile_counts_out);
    else
        hipLaunchKernelGGL((saturation::level_mask_tiles_kernel<1>), dim3(grid), dim3(kStreamThreads), 0, stream, levels, pixels, blocks_per_tile, tile_thresholds, mask_out, tile_counts_out);
    return check_launch("level mask");
}
