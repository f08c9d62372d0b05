// Tissue detection (included from reinhard.hip, where sx_tissue_mask lives): the 256-bin luminosity histogram an Otsu threshold is taken
// from, the rule with a cut per tile read on the device, and binary morphology on masks.  All three produce integers: every result is
// checked exactly.
//
// The histogram's bins are DEFINED by the rule: cut[k] = y_cut_of(k / 256) is the constant sx_tissue_mask compares a pixel's luminance Y
// with at luminosity_threshold = k / 256, and a pixel's bin is the number of k in 1..255 with !(Y < cut[k]).  So sum(counts[:k]) is
// exactly the tissue count of sx_tissue_mask at k / 256 -- same device function for Y, same host function for the constant -- and a
// NaN pixel (background under the rule at every threshold) lands in bin 255.
#pragma once

#include <algorithm>
#include <cmath>

#include "tissue.hpp"

namespace sx {
namespace detect {

constexpr int kBlocksPerTile = 64;      // as sx_tissue_mask: workgroup b takes share b % blocks_per_tile of tile b / blocks_per_tile
constexpr int kHistBins = 256;
constexpr int kHistCopies = 32;         // copies of the histogram in LDS, copy c in bank c (histmatch.hip: histogram_planar_kernel)

struct CutTable {
    float cut[kHistBins];               // cut[k], k = 1..255, strictly increasing; cut[0] is not read
};

template <typename T, int V>
__device__ __forceinline__ void load_pixels(const T* __restrict__ img, int64_t p, int64_t pixels, int64_t step, int64_t plane, T (&v)[3][V]) {
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
}

// The number of k in 1..255 with !(y < cut[k]): the cuts increase, so the k that hold are 1..K and eight compares find K.  NaN: every
// compare holds, bin 255.
__device__ __forceinline__ uint32_t bin_of(float y, const float* cut) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t s = kHistBins / 2; s > 0; s >>= 1)
        if (!(y < cut[lo + s])) lo += s;
    return lo;
}

// One memset and this launch.  A lane owns copy (lane % 32) of the workgroup's histogram, so the lanes of one LDS atomic instruction
// never share a bank but with their partner 32 lanes on; and a lane counts a run of equal bins itself and adds once per run (a glass
// tile puts nearly every pixel into two or three bins: 64 lanes adding 1 to the same few words would take their turns, pixel by pixel).
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void luminosity_histogram_kernel(const T* __restrict__ images, int64_t pixels, int channels_last, int blocks_per_tile, int pooled, CutTable cuts, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t hist[kHistBins][kHistCopies];
    __shared__ float cut[kHistBins];
    __shared__ LinearTable table;
    for (int i = threadIdx.x; i < kHistBins * kHistCopies; i += kStreamThreads) (&hist[0][0])[i] = 0;
    for (int i = threadIdx.x; i < kHistBins; i += kStreamThreads) cut[i] = cuts.cut[i];
    if constexpr (sizeof(T) == 1) table.fill();
    __syncthreads();
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;      // element (p, c) of a tile: p * step + c * plane
    uint32_t* mine = &hist[0][threadIdx.x & (kHistCopies - 1)];
    uint32_t last = 0, run = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        T v[3][V];
        load_pixels<T, V>(img, p, pixels, step, plane, v);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint32_t b = bin_of(tissue::luminance(tissue::linear_of<T>(v[0][i], table), tissue::linear_of<T>(v[1][i], table), tissue::linear_of<T>(v[2][i], table)), cut);
            if (b == last) {
                ++run;
            } else {
                if (run) atomicAdd(&mine[last * kHistCopies], run);
                last = b;
                run = 1;
            }
        }
    }
    if (run) atomicAdd(&mine[last * kHistCopies], run);
    __syncthreads();
    for (int t = threadIdx.x; t < kHistBins; t += kStreamThreads) {      // thread t adds up the copies of bin t, starting at its own bank
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < kHistCopies; ++k) sum += hist[t][(t + k) & (kHistCopies - 1)];
        if (sum) atomicAdd(&counts[(pooled ? 0 : tile) * kHistBins + t], sum);
    }
}

template <typename T>
static int run_histogram(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, int pooled, unsigned long long* counts, hipStream_t stream) {
    const int64_t pixels = h * w;
    CutTable cuts;
    cuts.cut[0] = 0.0f;
    for (int k = 1; k < kHistBins; ++k) cuts.cut[k] = tissue::y_cut_of(k / 256.0);
    if (hipMemsetAsync(counts, 0, sizeof(unsigned long long) * kHistBins * (size_t)(pooled ? 1 : n), stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    const bool vec = !channels_last && pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0;
    const int per_block = kStreamThreads * (vec ? 4 : 1);
    const int blocks_per_tile = (int)std::min<int64_t>((pixels + per_block - 1) / per_block, kBlocksPerTile);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((luminosity_histogram_kernel<T, 4>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, pooled, cuts, counts);
    else
        hipLaunchKernelGGL((luminosity_histogram_kernel<T, 1>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, pooled, cuts, counts);
    return check_launch("luminosity histogram");
}

// sx_tissue_mask_tiles: tissue_mask_kernel (reinhard.hip) with the constant of tile i read from device memory -- the same grid, the same
// loads, the same device function, so equal cuts give the bits of sx_tissue_mask.  A NaN cut: no compare holds, an empty tile.
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void tissue_mask_tiles_kernel(const T* __restrict__ images, int64_t pixels, int channels_last, int blocks_per_tile, const float* __restrict__ tile_y_cut, uint8_t* __restrict__ mask_out, unsigned long long* __restrict__ counts_out) {
    __shared__ LinearTable table;
    if constexpr (sizeof(T) == 1) table.fill();
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const float y_cut = tile_y_cut[tile];
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;
    unsigned int mine = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        T v[3][V];
        load_pixels<T, V>(img, p, pixels, step, plane, v);
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
static int run_mask_tiles(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, const float* tile_y_cut, uint8_t* mask_out, unsigned long long* counts_out, hipStream_t stream) {
    const int64_t pixels = h * w;
    if (counts_out && hipMemsetAsync(counts_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    const bool vec = !channels_last && pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0 && reinterpret_cast<uintptr_t>(mask_out) % 4 == 0;
    const int per_block = kStreamThreads * (vec ? 4 : 1);
    const int blocks_per_tile = (int)std::min<int64_t>((pixels + per_block - 1) / per_block, kBlocksPerTile);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((tissue_mask_tiles_kernel<T, 4>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, tile_y_cut, mask_out, counts_out);
    else
        hipLaunchKernelGGL((tissue_mask_tiles_kernel<T, 1>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, tile_y_cut, mask_out, counts_out);
    return check_launch("tissue mask (per-tile cuts)");
}

// ---- binary morphology -----------------------------------------------------------------------------------------------------------
// A workgroup writes kMorphRows x 64 pixels of one tile.  It stages the rows it needs, halo included, ON CHIP ONCE, a bit per pixel: a
// wave takes a row of 64 columns, one lane per column, and __ballot packs it into a word; a staged row is three words (the 64 columns
// to the left, the workgroup's own, the 64 to the right: a radius of up to 63 would fit).  Only erosion is computed: a dilation is the
// erosion of the complement (the elements are symmetric), so its bits are staged and written complemented.  What lies outside the tile
// is staged as 1 -- "set" for an erosion, "unset" for a dilation: it never constrains the result, and tiles never see each other.
// Thread t then owns output row t: the erosion by the element is the AND over dy of the horizontal erosion of half-width half[|dy|] of
// row t + dy; rows that share a half-width are ANDed first and eroded once (erosions commute with AND), so a square costs one
// horizontal erosion per row and a disk one per distinct half-width.  A horizontal erosion of a 192-bit row is a window AND by
// doubling: B_1 = row, B_2m(i) = B_m(i) & B_m(i + m), and the window of 2h + 1 bits around i is B_p(i - h) & B_p(i + h + 1 - p).
constexpr int kMorphRows = 256;
constexpr int kMorphCols = 64;
constexpr int kMorphMaxRadius = SX_MORPH_MAX_RADIUS;
static_assert(kMorphMaxRadius < 32, "the doubling below shifts by at most 16 and the halo words hold 64 columns");

struct HalfWidths {
    uint8_t half[kMorphMaxRadius + 2];      // half[|dy|], |dy| = 0..radius: non-increasing
};

// 64 bits from bit `pos` (0 < pos < 128) of the 192-bit row w0 | w1 << 64 | w2 << 128
__device__ __forceinline__ uint64_t window64(uint64_t w0, uint64_t w1, uint64_t w2, int pos) {
    if (pos < 64) return (w0 >> pos) | (w1 << (64 - pos));
    pos -= 64;
    return pos == 0 ? w1 : (w1 >> pos) | (w2 << (64 - pos));
}

// bits 64..127 of the row eroded horizontally by half-width h (0..31); beyond bit 191 the row reads as set
__device__ __forceinline__ uint64_t erode_row(uint64_t w0, uint64_t w1, uint64_t w2, int h) {
    const int n = 2 * h + 1;
    int m = 1;
    while (2 * m <= n) {
        w0 &= (w0 >> m) | (w1 << (64 - m));
        w1 &= (w1 >> m) | (w2 << (64 - m));
        w2 &= (w2 >> m) | (~0ull << (64 - m));
        m *= 2;
    }
    return window64(w0, w1, w2, 64 - h) & window64(w0, w1, w2, 64 + h + 1 - m);
}

__global__ __launch_bounds__(kMorphRows) void morphology_kernel(const uint8_t* __restrict__ mask_in, uint8_t* __restrict__ mask_out, int64_t height, int64_t width, int row_blocks, int col_blocks, int radius, int dilate, HalfWidths halves, unsigned long long* __restrict__ counts_out) {
    __shared__ uint64_t staged[kMorphRows + 2 * kMorphMaxRadius][3];
    __shared__ uint64_t result[kMorphRows];
    const int per_tile = row_blocks * col_blocks;
    const int64_t tile = blockIdx.x / per_tile;
    const int within = blockIdx.x % per_tile;
    const int64_t y0 = (int64_t)(within / col_blocks) * kMorphRows, x0 = (int64_t)(within % col_blocks) * kMorphCols;
    const uint8_t* src = mask_in + tile * height * width;
    uint8_t* dst = mask_out + tile * height * width;
    const int rows_out = (int)min((int64_t)kMorphRows, height - y0);
    const int wave = threadIdx.x / kWave, lane = (int)lane_id();
    for (int j = wave; j < (rows_out + 2 * radius) * 3; j += kMorphRows / kWave) {      // (uniform in a wave: every lane votes)
        const int row = j / 3, word = j % 3;
        const int64_t gy = y0 - radius + row, gx = x0 + (word - 1) * kMorphCols + lane;
        bool bit = true;
        if (gy >= 0 && gy < height && gx >= 0 && gx < width && gx >= x0 - radius && gx < x0 + kMorphCols + radius) bit = (src[gy * width + gx] != 0) != (dilate != 0);
        const uint64_t bits = __ballot(bit);
        if (lane == 0) staged[row][word] = bits;
    }
    __syncthreads();
    const int t = threadIdx.x;
    uint64_t res = 0;
    if (t < rows_out) {
        res = ~0ull;
        uint64_t a0 = ~0ull, a1 = ~0ull, a2 = ~0ull;
        for (int a = 0; a <= radius; ++a) {
            const uint64_t* up = staged[t + radius - a];
            const uint64_t* down = staged[t + radius + a];
            a0 &= up[0] & down[0];
            a1 &= up[1] & down[1];
            a2 &= up[2] & down[2];
            if (a == radius || halves.half[a + 1] != halves.half[a]) {
                res &= erode_row(a0, a1, a2, halves.half[a]);
                a0 = a1 = a2 = ~0ull;
            }
        }
        if (dilate) res = ~res;
        const int64_t cols = width - x0;
        if (cols < kMorphCols) res &= (1ull << cols) - 1ull;
    }
    result[t] = res;
    if (counts_out) {
        const unsigned int total = wave_total_u32((uint32_t)__popcll(res));
        if (lane == 0 && total) atomicAdd(&counts_out[tile], (unsigned long long)total);
    }
    __syncthreads();
    if (x0 + lane < width)
        for (int row = wave; row < rows_out; row += kMorphRows / kWave) dst[(y0 + row) * width + x0 + lane] = (uint8_t)((result[row] >> lane) & 1ull);
}

static bool morphology_grid(int64_t n, int64_t h, int64_t w, int* row_blocks, int* col_blocks, unsigned* grid) {
    const int64_t rb = (h + kMorphRows - 1) / kMorphRows, cb = (w + kMorphCols - 1) / kMorphCols;
    if (rb > 0x7fffffffll || cb > 0x7fffffffll || rb * cb > 0x7fffffffll || n > 0x7fffffffll / (rb * cb)) return false;
    *row_blocks = (int)rb;
    *col_blocks = (int)cb;
    *grid = (unsigned)(n * rb * cb);
    return true;
}

static void morphology_pass(const uint8_t* in, uint8_t* out, int64_t n, int64_t h, int64_t w, int radius, int element, int dilate, unsigned long long* counts, hipStream_t stream) {
    HalfWidths halves{};
    for (int a = 0; a <= radius; ++a) {
        int half = radius;
        if (element == SX_ELEMENT_DISK) {
            half = 0;
            while ((half + 1) * (half + 1) + a * a <= radius * radius) ++half;      // floor(sqrt(r^2 - a^2)), in integers
        }
        halves.half[a] = (uint8_t)half;
    }
    int row_blocks = 1, col_blocks = 1;
    unsigned grid = 0;
    morphology_grid(n, h, w, &row_blocks, &col_blocks, &grid);
    hipLaunchKernelGGL(morphology_kernel, dim3(grid), dim3(kMorphRows), 0, stream, in, out, h, w, row_blocks, col_blocks, radius, dilate, halves, counts);
}

}  // namespace detect
}  // namespace sx

extern "C" float sx_tissue_y_cut(double luminosity_threshold) {
    return sx::tissue::threshold_ok(luminosity_threshold) ? sx::tissue::y_cut_of(luminosity_threshold) : NAN;
}

extern "C" int sx_luminosity_histogram(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int pooled, unsigned long long* counts_out, void* stream_ptr) {
    using namespace sx;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!counts_out) return fail(SX_ERR_BAD_ARG, "counts_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return detect::run_histogram<typename decltype(t)::type>(images, n, h, w, channels_last, pooled != 0, counts_out, stream); });
}

extern "C" int sx_tissue_mask_tiles(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* tile_y_cut, uint8_t* mask_out, unsigned long long* tile_counts_out, void* stream_ptr) {
    using namespace sx;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!mask_out && !tile_counts_out) return fail(SX_ERR_BAD_ARG, "mask_out and tile_counts_out are both null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    if (!tile_y_cut) return fail(SX_ERR_BAD_ARG, "tile_y_cut pointer is null");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return detect::run_mask_tiles<typename decltype(t)::type>(images, n, h, w, channels_last, tile_y_cut, mask_out, tile_counts_out, stream); });
}

extern "C" int sx_mask_morphology(const uint8_t* mask_in, uint8_t* mask_out, int64_t n, int64_t h, int64_t w, int op, int element, int radius, uint8_t* scratch, unsigned long long* tile_counts_out, void* stream_ptr) {
    using namespace sx;
    if (!mask_in || !mask_out) return fail(SX_ERR_BAD_ARG, "mask_in / mask_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "masks must have positive sizes");
    if (op != SX_MORPH_ERODE && op != SX_MORPH_DILATE && op != SX_MORPH_OPEN && op != SX_MORPH_CLOSE) return fail(SX_ERR_BAD_ARG, "unknown morphology op %d", op);
    if (element != SX_ELEMENT_SQUARE && element != SX_ELEMENT_DISK) return fail(SX_ERR_BAD_ARG, "unknown structuring element %d", element);
    if (radius < 1 || radius > SX_MORPH_MAX_RADIUS) return fail(SX_ERR_BAD_ARG, "radius must lie in 1..%d, got %d", SX_MORPH_MAX_RADIUS, radius);
    if (mask_out == mask_in) return fail(SX_ERR_BAD_ARG, "mask_out must not be mask_in: the operation is not in place");
    const bool two = op == SX_MORPH_OPEN || op == SX_MORPH_CLOSE;
    if (two && !scratch) return fail(SX_ERR_BAD_ARG, "open / close need a scratch of n_tiles x height x width bytes");
    if (two && (scratch == mask_in || scratch == mask_out)) return fail(SX_ERR_BAD_ARG, "scratch must be neither mask_in nor mask_out");
    int row_blocks = 0, col_blocks = 0;
    unsigned grid = 0;
    if (!detect::morphology_grid(n, h, w, &row_blocks, &col_blocks, &grid)) return fail(SX_ERR_BAD_ARG, "masks too large for one call");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if (tile_counts_out && hipMemsetAsync(tile_counts_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    if (!two) {
        detect::morphology_pass(mask_in, mask_out, n, h, w, radius, element, op == SX_MORPH_DILATE, tile_counts_out, stream);
    } else {
        const int first_dilates = op == SX_MORPH_CLOSE;
        detect::morphology_pass(mask_in, scratch, n, h, w, radius, element, first_dilates, nullptr, stream);
        detect::morphology_pass(scratch, mask_out, n, h, w, radius, element, !first_dilates, tile_counts_out, stream);
    }
    return check_launch("mask morphology");
}
