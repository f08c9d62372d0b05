// Focus measurement (included from reinhard.hip beside saturation.hpp, whose level rule and streaming grid the kernels here share): the
// grey level of a batch as an 8-bit map, the integer sums behind the Laplacian variance and the Tenengrad per tile, per cell of a grid
// or per batch, and the expansion of a cell grid to a pixel mask.  Every result is an integer and every definition exact.
//
// The grey level of a pixel with 8-bit levels r, g, b (saturation::level_of): Y = (4899 r + 9617 g + 1868 b + 8192) >> 14, the
// fixed-point rule of an 8-bit RGB -> grey conversion; the weights sum to 16384, so Y lies in 0..255.  A pixel with a NaN in any channel
// has Y = 0.  The stencils read Y with the border reflected WITHOUT repeating the edge (-1 -> 1, H -> H - 2; an axis of length 1 maps to
// 0), inside the pixel's own tile:
//   L  = Y[y-1,x] + Y[y+1,x] + Y[y,x-1] + Y[y,x+1] - 4 Y[y,x]                                   |L|  <= 1020
//   Gx = (Y[y-1,x+1] + 2 Y[y,x+1] + Y[y+1,x+1]) - (Y[y-1,x-1] + 2 Y[y,x-1] + Y[y+1,x-1])        |Gx| <= 1020
//   Gy = (Y[y+1,x-1] + 2 Y[y+1,x] + Y[y+1,x+1]) - (Y[y-1,x-1] + 2 Y[y-1,x] + Y[y-1,x+1])        |Gy| <= 1020
//   T  = Gx^2 + Gy^2 <= 2 080 800
// A cell's statistics are four 64-bit words: pixels, sum L (signed, added as a two's-complement word), sum L^2, sum T.
#pragma once

#include <algorithm>
#include <type_traits>

#include "saturation.hpp"

namespace sx {
namespace focus {

template <typename T>
__device__ __forceinline__ uint8_t grey_of(T r, T g, T b) {
    bool nan = false;
    const int lr = saturation::level_of<T>(r, nan), lg = saturation::level_of<T>(g, nan), lb = saturation::level_of<T>(b, nan);
    if (nan) return 0;
    return (uint8_t)((uint32_t)(4899 * lr + 9617 * lg + 1868 * lb + 8192) >> 14);
}

// The grid, loads and layouts of saturation::saturation_map_kernel.
template <typename T, int V>
__global__ __launch_bounds__(kStreamThreads) void grey_map_kernel(const T* __restrict__ images, int64_t pixels, int channels_last, int blocks_per_tile, uint8_t* __restrict__ out) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        T v[3][V];
        detect::load_pixels<T, V>(img, p, pixels, step, plane, v);
        uint8_t s[V];
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = grey_of<T>(v[0][i], v[1][i], v[2][i]);
        store_pack<uint8_t, V>(out + tile * pixels + p, s);
    }
}

template <typename T>
static int run_grey_map(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, uint8_t* out, hipStream_t stream) {
    const int64_t pixels = h * w;
    const bool vec = !channels_last && pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const int blocks_per_tile = saturation::level_blocks_per_tile(pixels, vec);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((grey_map_kernel<T, 4>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, out);
    else
        hipLaunchKernelGGL((grey_map_kernel<T, 1>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), pixels, channels_last, blocks_per_tile, out);
    return check_launch("grey map");
}

// ---- the statistics ----------------------------------------------------------------------------------------------------------------
// A workgroup takes kFocusRows x kFocusCols pixels of one tile.  It stages their grey levels with a one-pixel halo ON CHIP ONCE, a byte
// per pixel, computing each from the stored elements as it stages; every coordinate is reflected into the tile as it is staged, so the
// border rule costs nothing later, no load leaves the tile and tiles never see each other.  On aligned planar input a lane loads a pack
// of four pixels per channel and writes their four grey levels as one word; the halo columns, unaligned views and NHWC take single
// elements.  A staged row is kFocusStride bytes: three bytes of padding, the left halo column, the 64 columns, and the right halo
// column in the first padding byte of the next row -- the 64 columns start on a word, and 68 bytes put the two rows that the 32 lanes of
// a ds_write_b32 group write 17 banks apart (one shared bank of 32).  The reads of the second phase are consecutive bytes.
//
// Then a wave takes kFocusBand consecutive rows and a lane a column.  The lane keeps three rows of its column's neighbourhood in
// registers -- of each row the smoothed value l + 2 m + r, the difference r - l and m itself -- and slides down, one row of three byte
// reads per output row.  It accumulates pixels, L, L^2 and T in 32-bit registers for at most kFocusBand rows; then the lanes are added
// up by one prefix sum per word (wave_scan_u32), cut at the cell boundaries for cells narrower than the row: the sum of a segment is the
// difference of two prefix sums, exact modulo 2^32 and below 2^32 by the bound asserted here.  The segment's last lane adds the four
// sums to the workgroup's copy of its cell in LDS (64-bit integer adds; sum L sign-extended: two's complement adds in any order).
//
// Last the workgroup writes its cells: a cell that lies inside the workgroup's block (both sides <= 64) with plain stores -- every cell
// of the grid lies in exactly one block, so the output needs no clearing -- and a cell that spans workgroups with one 64-bit integer
// add per workgroup and word into the cleared output.
constexpr int kFocusRows = 64;
constexpr int kFocusCols = 64;
constexpr int kFocusThreads = 256;
constexpr int kFocusWaves = kFocusThreads / kWave;
constexpr int kFocusBand = kFocusRows / kFocusWaves;                  // rows a wave takes, and the most a lane accumulates in 32 bits
constexpr int kFocusStride = kFocusCols + 4;                          // bytes of a staged row
constexpr int kFocusStagedRows = kFocusRows + 2;
constexpr int kFocusStagedCols = kFocusCols + 2;
constexpr int kFocusFirst = 4;                                        // the byte of a staged row that holds the block's first column
constexpr int kFocusMinSide = 8;
constexpr int kFocusMaxCells = (kFocusRows / kFocusMinSide) * (kFocusCols / kFocusMinSide);
constexpr int kFocusWords = 4;                                        // pixels, sum L, sum L^2, sum T
constexpr unsigned long long kFocusMaxT = 2ull * 1020ull * 1020ull;   // Gx^2 + Gy^2
static_assert(kFocusCols == kWave && kFocusRows % kFocusWaves == 0, "a wave takes a band of rows, a lane a column");
static_assert((unsigned long long)kFocusBand * kWave * kFocusMaxT < (1ull << 32), "the sum T of a band's rows over a whole wave fits 32 bits (so does every segment of it, and sum L^2 <= sum T / 2)");
static_assert(kFocusBand % kFocusMinSide == 0 && kFocusMaxCells * kFocusWords <= kFocusThreads, "cells nest in bands or bands in cells; a thread writes one word of one cell");
static_assert(kFocusFirst % 4 == 0 && kFocusStride % 4 == 0 && kFocusFirst + kFocusCols == kFocusStride, "packs are stored as words; the right halo is byte 0 of the next row");

struct FocusArgs {
    int64_t height, width;
    int64_t block_h, block_w;        // the cell; the whole tile: height and width rounded up to the block (one cell, gh = gw = 1)
    int64_t grid_h, grid_w;          // cells per tile
    int row_blocks, col_blocks;      // workgroups per tile
    int channels_last, pooled, plain, mask_vec;
    unsigned long long* out;         // kFocusWords planes of n_tiles x grid_h x grid_w words (pooled: of one word)
    int64_t cells;                   // words per plane
};

// the coordinate q of an axis of length n read with the reflected border; only -1 <= q <= n matters, anything else lands somewhere inside
__device__ __forceinline__ int64_t reflect(int64_t q, int64_t n) {
    q = q < 0 ? -q : q;
    q = q >= n ? 2 * n - 2 - q : q;
    return min(max(q, (int64_t)0), n - 1);
}

template <typename T>
__device__ __forceinline__ uint8_t grey_at(const T* __restrict__ img, int64_t p, int64_t step, int64_t plane) {
    return grey_of<T>(img[p * step], img[p * step + plane], img[p * step + 2 * plane]);
}

template <typename T, int V, bool kMask>
__global__ __launch_bounds__(kFocusThreads) void focus_statistics_kernel(const T* __restrict__ images, const uint8_t* __restrict__ mask, FocusArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t grey[kFocusStagedRows * kFocusStride + 4];
    __shared__ __attribute__((aligned(16))) uint8_t inside[kMask ? kFocusRows * kFocusCols : 4];
    __shared__ unsigned long long acc[kFocusMaxCells][kFocusWords];
    const int tid = threadIdx.x;
    const int per_tile = a.row_blocks * a.col_blocks;
    const int64_t tile = blockIdx.x / per_tile;
    const int within = blockIdx.x % per_tile;
    const int64_t y0 = (int64_t)(within / a.col_blocks) * kFocusRows, x0 = (int64_t)(within % a.col_blocks) * kFocusCols;
    const int64_t height = a.height, width = a.width, pixels = height * width;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = a.channels_last ? 1 : pixels, step = a.channels_last ? 3 : 1;
    if (tid < kFocusMaxCells * kFocusWords) (&acc[0][0])[tid] = 0ull;      // (at most kFocusThreads words: asserted)

    // ---- stage the grey levels
    if constexpr (V == 4) {
        constexpr int kPacks = kFocusCols / 4, kItems = kFocusStagedRows * kPacks;
#pragma unroll
        for (int k = 0; k < (kItems + kFocusThreads - 1) / kFocusThreads; ++k) {
            const int i = k * kFocusThreads + tid;
            if (i < kItems) {
                const int sr = i / kPacks, j = i % kPacks;
                const int64_t gy = reflect(y0 - 1 + sr, height), gx = x0 + 4 * j;
                uint8_t y[4] = {0, 0, 0, 0};
                if (gx < width) {      // (width % 4 == 0: the pack lies inside the row)
                    T v[3][4];
                    detect::load_pixels<T, 4>(img, gy * width + gx, pixels, step, plane, v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = grey_of<T>(v[0][e], v[1][e], v[2][e]);
                } else {               // beyond the tile: column `width` is the right neighbour of the last column, the rest is not read for a result
                    y[0] = grey_at<T>(img, gy * width + reflect(gx, width), step, plane);
                }
                store_pack<uint8_t, 4>(&grey[sr * kFocusStride + kFocusFirst + 4 * j], y);
            }
        }
        if (tid < 2 * kFocusStagedRows) {      // the halo columns
            const int sr = tid >> 1, right = tid & 1;
            const int64_t gy = reflect(y0 - 1 + sr, height), gx = reflect(right ? x0 + kFocusCols : x0 - 1, width);
            grey[sr * kFocusStride + kFocusFirst + (right ? kFocusCols : -1)] = grey_at<T>(img, gy * width + gx, step, plane);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < kFocusStagedRows * kFocusStagedCols; i += kFocusThreads) {
            const int sr = i / kFocusStagedCols, sc = i % kFocusStagedCols;
            const int64_t gy = reflect(y0 - 1 + sr, height), gx = reflect(x0 - 1 + sc, width);
            grey[sr * kFocusStride + kFocusFirst - 1 + sc] = grey_at<T>(img, gy * width + gx, step, plane);
        }
    }
    if constexpr (kMask) {      // the block's mask bytes; 0 outside the tile
        const uint8_t* msk = mask + tile * pixels;
        if (a.mask_vec) {       // (width % 4 == 0 and the mask on a word)
            constexpr int kPacks = kFocusCols / 4;
#pragma unroll
            for (int k = 0; k < kFocusRows * kPacks / kFocusThreads; ++k) {
                const int i = k * kFocusThreads + tid;
                const int r = i / kPacks, j = i % kPacks;
                const int64_t gy = y0 + r, gx = x0 + 4 * j;
                uint32_t word = 0;
                if (gy < height && gx < width) word = *reinterpret_cast<const uint32_t*>(msk + gy * width + gx);
                *reinterpret_cast<uint32_t*>(&inside[r * kFocusCols + 4 * j]) = word;
            }
        } else {
            for (int i = tid; i < kFocusRows * kFocusCols; i += kFocusThreads) {
                const int64_t gy = y0 + i / kFocusCols, gx = x0 + i % kFocusCols;
                inside[i] = (gy < height && gx < width) ? msk[gy * width + gx] : (uint8_t)0;
            }
        }
    }
    __syncthreads();

    // ---- a wave a band of rows, a lane a column
    const int lane = tid % kWave, wave = tid / kWave;
    const int cell_rows = (int)min(a.block_h, (int64_t)kFocusRows), cell_cols = (int)min(a.block_w, (int64_t)kFocusCols);      // the cell inside the block
    const int flush_rows = min(cell_rows, kFocusBand), cells_across = kFocusCols / cell_cols;
    const bool column_in = x0 + lane < width;
    const int first_row = wave * kFocusBand;
    const uint8_t* mine = &grey[kFocusFirst - 1 + lane];      // mine[sr * kFocusStride + 0 / 1 / 2]: left, middle, right of staged row sr
    int s_up, d_up, m_up, s_at, d_at, m_at, side_at;
    {
        const uint8_t* row = mine + first_row * kFocusStride;
        const int l = row[0], m = row[1], r = row[2];
        s_up = l + 2 * m + r, d_up = r - l, m_up = m;
        row += kFocusStride;
        const int l1 = row[0], m1 = row[1], r1 = row[2];
        s_at = l1 + 2 * m1 + r1, d_at = r1 - l1, m_at = m1, side_at = l1 + r1;
    }
    uint32_t count = 0, sum_l = 0, sum_l2 = 0, sum_t = 0;
    for (int row_in = first_row; row_in < first_row + kFocusBand; ++row_in) {
        const uint8_t* row = mine + (row_in + 2) * kFocusStride;
        const int l = row[0], m = row[1], r = row[2];
        const int s_dn = l + 2 * m + r, d_dn = r - l;
        const int lap = m_up + m + side_at - 4 * m_at;
        const int gx = d_up + 2 * d_at + d_dn, gy = s_dn - s_up;
        bool in = column_in && y0 + row_in < height;
        if constexpr (kMask) in = in && inside[row_in * kFocusCols + lane] != 0;
        if (in) {
            count += 1u;
            sum_l += (uint32_t)lap;
            sum_l2 += (uint32_t)(lap * lap);
            sum_t += (uint32_t)(gx * gx + gy * gy);
        }
        s_up = s_at, d_up = d_at, m_up = m_at;
        s_at = s_dn, d_at = d_dn, m_at = m, side_at = l + r;
        if ((row_in + 1) % flush_rows == 0) {      // (uniform in the workgroup) the end of a cell's rows in this band, or of the band
            const uint32_t scan[kFocusWords] = {wave_scan_u32(count), wave_scan_u32(sum_l), wave_scan_u32(sum_l2), wave_scan_u32(sum_t)};
            uint32_t total[kFocusWords];
#pragma unroll
            for (int k = 0; k < kFocusWords; ++k) {
                const uint32_t before = (uint32_t)__shfl((int)scan[k], (lane - cell_cols) & (kWave - 1), kWave);      // (every lane takes part)
                total[k] = scan[k] - (lane >= cell_cols ? before : 0u);
            }
            if (lane % cell_cols == cell_cols - 1 && total[0] != 0u) {
                unsigned long long* cell = acc[(row_in / cell_rows) * cells_across + lane / cell_cols];
                atomicAdd(&cell[0], (unsigned long long)total[0]);
                atomicAdd(&cell[1], (unsigned long long)(long long)(int32_t)total[1]);
                atomicAdd(&cell[2], (unsigned long long)total[2]);
                atomicAdd(&cell[3], (unsigned long long)total[3]);
            }
            count = sum_l = sum_l2 = sum_t = 0;
        }
    }
    __syncthreads();

    // ---- a thread a word of a cell
    const int cell = tid / kFocusWords, word = tid % kFocusWords;
    if (cell < (kFocusRows / cell_rows) * cells_across) {
        const int64_t cy0 = y0 + (int64_t)(cell / cells_across) * cell_rows, cx0 = x0 + (int64_t)(cell % cells_across) * cell_cols;
        if (cy0 < height && cx0 < width) {
            const int64_t index = a.pooled ? 0 : (tile * a.grid_h + cy0 / a.block_h) * a.grid_w + cx0 / a.block_w;
            const unsigned long long value = acc[cell][word];
            if (a.plain)
                a.out[word * a.cells + index] = value;
            else if (value)
                atomicAdd(&a.out[word * a.cells + index], value);
        }
    }
}

// The zeroes of a call on a stream that is being captured: a clearing launch instead of the memset (the rule of sx_deconv_moments).
__global__ void focus_clear_kernel(unsigned long long* __restrict__ out, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) out[i] = 0ull;
}

static int clear_words(unsigned long long* out, int64_t words, hipStream_t stream) {
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipStreamIsCapturing failed");
    if (capture == hipStreamCaptureStatusNone) {
        if (hipMemsetAsync(out, 0, (size_t)words * sizeof(unsigned long long), stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
        return SX_OK;
    }
    hipLaunchKernelGGL(focus_clear_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, out, words);
    return check_launch("focus (clear)");
}

template <typename T, bool kMask>
static int run_focus_statistics(const void* images, const uint8_t* mask, int64_t n, FocusArgs a, unsigned grid, hipStream_t stream) {
    const bool vec = !a.channels_last && a.width % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0;
    a.mask_vec = kMask && a.width % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
    if (vec)
        hipLaunchKernelGGL((focus_statistics_kernel<T, 4, kMask>), dim3(grid), dim3(kFocusThreads), 0, stream, static_cast<const T*>(images), mask, a);
    else
        hipLaunchKernelGGL((focus_statistics_kernel<T, 1, kMask>), dim3(grid), dim3(kFocusThreads), 0, stream, static_cast<const T*>(images), mask, a);
    return check_launch("focus statistics");
}

static bool side_ok(int64_t side) { return side == 8 || side == 16 || side == 32 || (side > 0 && side % 64 == 0); }

static int check_sides(int64_t block_h, int64_t block_w) {
    if (!side_ok(block_h) || !side_ok(block_w))
        return fail(SX_ERR_BAD_ARG, "block sides must each be 8, 16, 32, 64 or a multiple of 64, got (%lld, %lld)", (long long)block_h, (long long)block_w);
    return SX_OK;
}

template <bool kMask>
static int focus_statistics_call(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int64_t block_h, int64_t block_w, int pooled,
                                 const unsigned char* mask_dev, long long* out, void* stream_ptr) {
    int rc;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "statistics_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    const bool whole = block_h == 0 && block_w == 0;
    if (!whole && (rc = check_sides(block_h, block_w)) != SX_OK) return rc;
    if (pooled && !whole) return fail(SX_ERR_BAD_ARG, "pooled statistics take the whole tile as the cell (block 0 x 0), got (%lld, %lld)", (long long)block_h, (long long)block_w);
    FocusArgs a{};
    unsigned grid = 0;
    if (!saturation::median_grid(n, h, w, &a.row_blocks, &a.col_blocks, &grid)) return fail(SX_ERR_BAD_ARG, "images too large for one call");
    if ((rc = dtype_ok(dtype)) != SX_OK) return rc;      // (before anything is enqueued)
    a.height = h;
    a.width = w;
    a.block_h = whole ? (int64_t)a.row_blocks * kFocusRows : block_h;
    a.block_w = whole ? (int64_t)a.col_blocks * kFocusCols : block_w;
    a.grid_h = (h + a.block_h - 1) / a.block_h;
    a.grid_w = (w + a.block_w - 1) / a.block_w;
    a.channels_last = channels_last != 0;
    a.pooled = pooled != 0;
    a.plain = a.block_h <= kFocusRows && a.block_w <= kFocusCols && !pooled;
    a.out = reinterpret_cast<unsigned long long*>(out);
    a.cells = pooled ? 1 : n * a.grid_h * a.grid_w;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if (!a.plain && (rc = clear_words(a.out, a.cells * kFocusWords, stream)) != SX_OK) return rc;
    return with_dtype(dtype, [&](auto t) { return run_focus_statistics<typename decltype(t)::type, kMask>(images, mask_dev, n, a, grid, stream); });
}

// ---- a cell grid as a pixel mask: pixel = cell byte != 0 (and mask byte != 0); counts by wave sums as saturation::level_mask_tiles_kernel
template <int V>
__global__ __launch_bounds__(kStreamThreads) void cells_mask_kernel(const uint8_t* __restrict__ cells, const uint8_t* __restrict__ mask, int64_t width, int64_t pixels, int64_t block_h, int64_t block_w,
                                                                    int64_t grid_h, int64_t grid_w, int blocks_per_tile, uint8_t* __restrict__ mask_out, unsigned long long* __restrict__ counts_out) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const uint8_t* grid = cells + tile * grid_h * grid_w;
    unsigned int mine = 0;
    for (int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V; p < pixels; p += (int64_t)blocks_per_tile * kStreamThreads * V) {
        const int64_t y = p / width, x = p % width;      // (V == 4: width % 4 == 0 and the sides are multiples of 8: four pixels of one row and one cell)
        const bool on = grid[(y / block_h) * grid_w + x / block_w] != 0;
        uint8_t m[V];
        if (mask == nullptr) {
#pragma unroll
            for (int i = 0; i < V; ++i) m[i] = on ? 1 : 0;
        } else if constexpr (V == 1) {
            m[0] = (on && mask[tile * pixels + p] != 0) ? 1 : 0;
        } else {
            const Pack<uint8_t, V> pk = *reinterpret_cast<const Pack<uint8_t, V>*>(mask + tile * pixels + p);
#pragma unroll
            for (int i = 0; i < V; ++i) m[i] = (on && pk.v[i] != 0) ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) mine += m[i];
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

}  // namespace focus
}  // namespace sx

extern "C" int sx_grey_map(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, uint8_t* levels_out, void* stream_ptr) {
    using namespace sx;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!levels_out) return fail(SX_ERR_BAD_ARG, "levels_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return focus::run_grey_map<typename decltype(t)::type>(images, n, h, w, channels_last, levels_out, stream); });
}

extern "C" int sx_focus_statistics(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int64_t block_h, int64_t block_w, int pooled, long long* statistics_out,
                                   void* stream_ptr) {
    return sx::focus::focus_statistics_call<false>(images, dtype, n, h, w, channels_last, block_h, block_w, pooled, nullptr, statistics_out, stream_ptr);
}

extern "C" int sx_focus_statistics_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int64_t block_h, int64_t block_w, int pooled,
                                          const unsigned char* mask_dev, long long* statistics_out, void* stream_ptr) {
    return sx::focus::focus_statistics_call<true>(images, dtype, n, h, w, channels_last, block_h, block_w, pooled, mask_dev, statistics_out, stream_ptr);
}

extern "C" int sx_cells_mask(const uint8_t* cells, int64_t n, int64_t h, int64_t w, int64_t block_h, int64_t block_w, const unsigned char* mask_dev, uint8_t* mask_out,
                             unsigned long long* tile_counts_out, void* stream_ptr) {
    using namespace sx;
    int rc;
    if (!cells) return fail(SX_ERR_BAD_ARG, "cells pointer is null");
    if (!mask_out && !tile_counts_out) return fail(SX_ERR_BAD_ARG, "mask_out and tile_counts_out are both null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "masks must have positive sizes");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    if ((rc = focus::check_sides(block_h, block_w)) != SX_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const int64_t pixels = h * w;
    if (tile_counts_out && (rc = focus::clear_words(tile_counts_out, n, stream)) != SX_OK) return rc;
    const bool vec = w % 4 == 0 && reinterpret_cast<uintptr_t>(mask_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(mask_out) % 4 == 0;
    const int blocks_per_tile = saturation::level_blocks_per_tile(pixels, vec);
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    const int64_t grid_h = (h + block_h - 1) / block_h, grid_w = (w + block_w - 1) / block_w;
    if (vec)
        hipLaunchKernelGGL((focus::cells_mask_kernel<4>), dim3(grid), dim3(kStreamThreads), 0, stream, cells, mask_dev, w, pixels, block_h, block_w, grid_h, grid_w, blocks_per_tile, mask_out, tile_counts_out);
    else
        hipLaunchKernelGGL((focus::cells_mask_kernel<1>), dim3(grid), dim3(kStreamThreads), 0, stream, cells, mask_dev, w, pixels, block_h, block_w, grid_h, grid_w, blocks_per_tile, mask_out, tile_counts_out);
    return check_launch("cells mask");
}
