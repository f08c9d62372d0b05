// Connected components of masks and the area filters on them (included from reinhard.hip beside tissue_detect.hpp, whose block
// geometry and staging it shares).  Everything is integers: every result is checked exactly.
//
// The label of a set pixel is 1 + the raster index, within its tile, of the FIRST pixel of its component; unset pixels get 0.  That
// makes the labels a function of the mask alone.  The family is block-based union-find (Playne and Hawick; ECL-CC): a forest over the
// tile's pixels kept in `labels` as parent index + 1, in which a parent is never larger than its child, so the root of a component is
// its smallest index -- the canonical label.
//
//   1. components_local_kernel   a workgroup labels kLabelRows x 64 pixels of one tile ON CHIP, on row runs, and writes every set
//                                pixel's parent: the first pixel of its component WITHIN THE BLOCK.
//   2. components_seam_kernel    one thread per pixel along the seams between blocks unites across the seam.
//   3. components_flatten_kernel every pixel is pointed at its root; areas are added up at the roots, roots are counted.
//   4. area_filter_kernel        pixel-local: a pixel stays (or is filled) by the area found at its root.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so NO result here depends on
// a load seeing a store of another workgroup of the same launch.  Launch 1 writes disjoint blocks.  In launch 2 the forest changes
// under every thread's feet, and the only thing relied on is: (a) every value a word of `labels` has held since the launch began is
// an ancestor-or-self of that pixel in its component (parents only ever DECREASE, and only towards members of the same component), so a
// stale read walks to an older, still valid, member; and (b) the link itself is made by a RETURNING atomicMin on the word of the
// larger index, and what the atomic returns is the truth: if it was not a root any more the loop goes on with what it returned.
// Launch 3 runs after every union: roots are final, a non-root word holds an ancestor whether it is read before or after its owner
// rewrote it, and the walk ends at the true root either way.  No loop waits for another workgroup: every loop follows a value that
// strictly decreases by the thread's own loads and atomics.
#pragma once

#include "tissue_detect.hpp"

namespace sx {
namespace components {

constexpr int kLabelRows = detect::kMorphRows;      // 256: thread t owns row t of the block
constexpr int kLabelCols = detect::kMorphCols;      // 64: a row of the block is one 64-bit word
constexpr int kRunSlots = kLabelRows * kLabelCols / 2;      // two run starts of a row are at least two columns apart: start >> 1 is a slot of its own
constexpr int kFlatIters = 16;                      // flatten / filter: a wave takes 16 x 64 consecutive pixels of a tile
constexpr int kFlatPixels = kStreamThreads * kFlatIters;
static_assert(kLabelCols == kWave, "a row is staged by one wave with __ballot");

__device__ __forceinline__ uint64_t low_bits(int count) {      // count in 0..64
    return count >= 64 ? ~0ull : (1ull << count) - 1ull;
}
// first column of the run of set bits of `w` that holds bit `b`
__device__ __forceinline__ int run_start(uint64_t w, int b) {
    const uint64_t clear_below = ~w & low_bits(b);
    return clear_below ? 64 - __clzll((long long)clear_below) : 0;
}
// length of the run of set bits of `w` that starts at or holds bit `b`, counted from b
__device__ __forceinline__ int run_length_from(uint64_t w, int b) {
    const uint64_t inv = ~(w >> b);      // (b > 0: zeros came in at the top, inv != 0)
    return inv ? __ffsll((long long)inv) - 1 : 64;
}

// ---- the forest of a block in LDS: par[p >> 1] = parent of the run that starts at block pixel p = row * 64 + column -------------------
__device__ __forceinline__ uint32_t find_lds(const volatile uint32_t* par, uint32_t p) {
    for (;;) {
        const uint32_t q = par[p >> 1];
        if (q == p) return p;
        p = q;      // (q < p: ends)
    }
}
__device__ __forceinline__ void unite_lds(uint32_t* par, uint32_t a, uint32_t b) {
    a = find_lds(par, a);
    b = find_lds(par, b);
    while (a != b) {      // max(a, b) strictly decreases
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(&par[a >> 1], b);
        if (old == a) break;      // a was a root and hangs under b now
        a = old;                  // it was not: what it hung under and b remain to be united
    }
}

__global__ __launch_bounds__(kLabelRows) void components_local_kernel(const uint8_t* __restrict__ mask_in, int32_t* __restrict__ labels, int32_t* __restrict__ areas, int64_t height, int64_t width, int row_blocks, int col_blocks, int eight, int invert) {
    __shared__ uint64_t rows[kLabelRows];
    __shared__ uint32_t par[kRunSlots];
    const int per_tile = row_blocks * col_blocks;
    const int64_t tile = blockIdx.x / per_tile;
    const int within = blockIdx.x % per_tile;
    const int64_t y0 = (int64_t)(within / col_blocks) * kLabelRows, x0 = (int64_t)(within % col_blocks) * kLabelCols;
    const uint8_t* src = mask_in + tile * height * width;
    const int rows_in = (int)min((int64_t)kLabelRows, height - y0);
    const int wave = threadIdx.x / kWave, lane = (int)lane_id(), t = threadIdx.x;
    const bool in_cols = x0 + lane < width;
    for (int row = wave; row < kLabelRows; row += kLabelRows / kWave) {      // (uniform in a wave: every lane votes)
        bool bit = false;
        if (row < rows_in && in_cols) bit = (src[(y0 + row) * width + x0 + lane] != 0) != (invert != 0);
        const uint64_t bits = __ballot(bit);
        if (lane == 0) rows[row] = bits;
    }
    __syncthreads();
    const uint64_t w = rows[t];
    const uint64_t starts = w & ~(w << 1);
    for (uint64_t s = starts; s; s &= s - 1) {
        const uint32_t p = (uint32_t)(t * kLabelCols + __ffsll((long long)s) - 1);
        par[p >> 1] = p;
    }
    __syncthreads();
    const uint64_t up = t > 0 ? rows[t - 1] : 0ull;
    if (w && up) {
        for (uint64_t s = starts; s; s &= s - 1) {
            const int c = __ffsll((long long)s) - 1;
            const uint64_t run = low_bits(run_length_from(w, c)) << c;
            uint64_t touch = up & (eight ? (run | (run << 1) | (run >> 1)) : run);
            while (touch) {      // one union per run of the row above that this run touches
                const int b = __ffsll((long long)touch) - 1;
                touch &= ~(low_bits(run_length_from(up, b)) << b);
                unite_lds(par, (uint32_t)(t * kLabelCols + c), (uint32_t)((t - 1) * kLabelCols + run_start(up, b)));
            }
        }
    }
    __syncthreads();
    for (uint64_t s = starts; s; s &= s - 1) {      // (no union runs any more: roots are final, and any ancestor read on the way is valid)
        const uint32_t p = (uint32_t)(t * kLabelCols + __ffsll((long long)s) - 1);
        const uint32_t root = find_lds(par, p);
        if (root != p) par[p >> 1] = root;
    }
    __syncthreads();
    if (!in_cols) return;
    int32_t* dst = labels + tile * height * width;
    int32_t* area = areas ? areas + tile * height * width : nullptr;
    for (int row = wave; row < rows_in; row += kLabelRows / kWave) {
        const uint64_t bits = rows[row];
        int32_t label = 0;
        if ((bits >> lane) & 1ull) {
            const uint32_t root = par[(uint32_t)(row * kLabelCols + run_start(bits, lane)) >> 1];
            label = (int32_t)((y0 + (root >> 6)) * width + x0 + (root & 63u)) + 1;
        }
        const int64_t at = (y0 + row) * width + x0 + lane;
        dst[at] = label;
        if (area) area[at] = 0;
    }
}

// ---- the forest of a tile in global memory: labels[p] = parent index + 1 of a set pixel, 0 of an unset one ---------------------------
__device__ __forceinline__ int32_t find_global(int32_t* labels, int32_t p) {
    for (;;) {
        const int32_t q = __hip_atomic_load(&labels[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;      // (past the L1; an older value would do too)
        if (q == p) return p;
        p = q;
    }
}
__device__ __forceinline__ void unite_global(int32_t* labels, int32_t a, int32_t b) {
    a = find_global(labels, a);
    b = find_global(labels, b);
    while (a != b) {
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(&labels[a], b + 1) - 1;
        if (old == a) break;
        a = old;
    }
}

// A thread per pixel of the rows y = 256 k (k >= 1) and of the columns x = 64 k (k >= 1) of a tile: it unites its pixel with the
// neighbours across the seam.  A straight neighbour across the seam stands for the two diagonal ones beside it (they are its
// neighbours along the seam); without it the diagonal ones are united directly -- block corners included.  And a straight pair is
// left out where the pair before it along the seam is set too and lies in the same two blocks: on an all-set tile a seam of 64 or
// 256 pixels then costs one union, not one per pixel on the same root.
__global__ __launch_bounds__(kStreamThreads) void components_seam_kernel(int32_t* labels_all, int64_t height, int64_t width, int64_t seam_rows, int64_t seam_pixels, int blocks_per_tile, int eight) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    int64_t s = (int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x;
    if (s >= seam_pixels) return;
    int32_t* labels = labels_all + tile * height * width;
    const bool across_rows = s < seam_rows;      // the pixel lies in the first row of a block row: the seam is above it
    int64_t y, x;
    if (across_rows) {
        y = (s / width + 1) * kLabelRows;
        x = s % width;
    } else {
        s -= seam_rows;
        x = (s / height + 1) * kLabelCols;
        y = s % height;
    }
    auto set = [&](int64_t yy, int64_t xx) { return yy >= 0 && yy < height && xx >= 0 && xx < width && labels[yy * width + xx] != 0; };      // (0 or not never changes)
    if (!set(y, x)) return;
    const int32_t here = (int32_t)(y * width + x);
    if (across_rows) {
        if (set(y - 1, x)) {
            if (!(x % kLabelCols != 0 && set(y, x - 1) && set(y - 1, x - 1))) unite_global(labels, here, (int32_t)((y - 1) * width + x));
        } else if (eight) {
            if (set(y - 1, x - 1)) unite_global(labels, here, (int32_t)((y - 1) * width + x - 1));
            if (set(y - 1, x + 1)) unite_global(labels, here, (int32_t)((y - 1) * width + x + 1));
        }
    } else {
        if (set(y, x - 1)) {
            if (!(y % kLabelRows != 0 && set(y - 1, x) && set(y - 1, x - 1))) unite_global(labels, here, (int32_t)(y * width + x - 1));
        } else if (eight) {
            if (set(y - 1, x - 1)) unite_global(labels, here, (int32_t)((y - 1) * width + x - 1));
            if (set(y + 1, x - 1)) unite_global(labels, here, (int32_t)((y + 1) * width + x - 1));
        }
    }
}

// A wave takes kFlatIters x 64 consecutive pixels.  Areas: the lanes of a run of equal roots elect their first lane, which learns the
// run's length from the vote, and that lane keeps adding as long as ITS runs go on naming the same root (the luminosity histogram's
// run counting): a tile that is one component costs one atomic per wave, not one per pixel.
__global__ __launch_bounds__(kStreamThreads) void components_flatten_kernel(int32_t* labels_all, int32_t* areas_all, int64_t pixels, int blocks_per_tile, unsigned long long* __restrict__ tile_components) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    int32_t* labels = labels_all + tile * pixels;
    int32_t* areas = areas_all ? areas_all + tile * pixels : nullptr;
    const int lane = (int)lane_id();
    const int64_t base = (int64_t)(blockIdx.x % blocks_per_tile) * kFlatPixels + (int64_t)(threadIdx.x / kWave) * (kFlatIters * kWave);
    int32_t last = -1;
    uint32_t run = 0, roots = 0;
    for (int it = 0; it < kFlatIters && base + it * kWave < pixels; ++it) {      // (uniform in a wave)
        const int64_t p = base + it * kWave + lane;
        int32_t root = -1;
        if (p < pixels) {
            const int32_t mine = labels[p] - 1;
            if (mine >= 0) {
                root = mine;
                for (;;) {
                    const int32_t q = labels[root] - 1;
                    if (q == root) break;
                    root = q;
                }
                if (root != mine) labels[p] = root + 1;
                roots += root == (int32_t)p;
            }
        }
        const int32_t before = __shfl_up(root, 1, kWave);
        const bool head = lane == 0 || before != root;
        const uint64_t heads = __ballot(head);
        if (areas && head && root >= 0) {
            const uint64_t above = lane == kWave - 1 ? 0ull : heads & (~0ull << (lane + 1));
            const uint32_t length = (uint32_t)((above ? __ffsll((long long)above) - 1 : kWave) - lane);
            if (root == last) {
                run += length;
            } else {
                if (run) atomicAdd(&areas[last], (int32_t)run);
                last = root;
                run = length;
            }
        }
    }
    if (run) atomicAdd(&areas[last], (int32_t)run);
    if (tile_components) {
        const uint32_t total = wave_total_u32(roots);
        if (lane == 0 && total) atomicAdd(&tile_components[tile], (unsigned long long)total);
    }
}

// labels are flat, areas complete.  The labelled bit of a pixel (the mask's, or its complement's for holes) stays where its
// component has min_area pixels or more; the output is that bit for objects and its complement for holes, so
// holes(m) == 1 - objects(1 - m) holds by construction.
__global__ __launch_bounds__(kStreamThreads) void area_filter_kernel(const int32_t* __restrict__ labels_all, const int32_t* __restrict__ areas_all, uint8_t* __restrict__ mask_out, int64_t pixels, int blocks_per_tile, int holes, int64_t min_area, unsigned long long* __restrict__ counts_out) {
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const int32_t* labels = labels_all + tile * pixels;
    const int32_t* areas = areas_all + tile * pixels;
    uint8_t* dst = mask_out + tile * pixels;
    const int lane = (int)lane_id();
    const int64_t base = (int64_t)(blockIdx.x % blocks_per_tile) * kFlatPixels + (int64_t)(threadIdx.x / kWave) * (kFlatIters * kWave);
    uint32_t mine = 0;
    for (int it = 0; it < kFlatIters; ++it) {
        const int64_t p = base + it * kWave + lane;
        if (p >= pixels) break;
        const int32_t label = labels[p];
        const bool stays = label != 0 && (int64_t)areas[label - 1] >= min_area;
        const uint8_t bit = (uint8_t)(stays != (holes != 0));
        dst[p] = bit;
        mine += bit;
    }
    if (counts_out) {
        const uint32_t total = wave_total_u32(mine);
        if (lane == 0 && total) atomicAdd(&counts_out[tile], (unsigned long long)total);
    }
}

struct Grids {
    int row_blocks, col_blocks, seam_blocks, flat_blocks;
    unsigned local_grid, seam_grid, flat_grid;
    int64_t seam_rows, seam_pixels;
};

static bool grids_of(int64_t n, int64_t h, int64_t w, Grids* g) {
    unsigned grid = 0;
    if (!detect::morphology_grid(n, h, w, &g->row_blocks, &g->col_blocks, &grid)) return false;
    g->local_grid = grid;
    g->seam_rows = (int64_t)(g->row_blocks - 1) * w;
    g->seam_pixels = g->seam_rows + (int64_t)(g->col_blocks - 1) * h;
    const int64_t sb = (g->seam_pixels + kStreamThreads - 1) / kStreamThreads, fb = (h * w + kFlatPixels - 1) / kFlatPixels;
    if (sb > 0x7fffffffll / n || fb > 0x7fffffffll / n) return false;
    g->seam_blocks = (int)sb;
    g->flat_blocks = (int)fb;
    g->seam_grid = (unsigned)(n * sb);
    g->flat_grid = (unsigned)(n * fb);
    return true;
}

// launches 1 to 3 (the seam launch only where a tile has more than one block); tile_components, where given, was cleared by the caller
static void label_tiles(const uint8_t* mask_in, int64_t n, int64_t h, int64_t w, const Grids& g, int eight, int invert, int32_t* labels, int32_t* areas, unsigned long long* tile_components, hipStream_t stream) {
    hipLaunchKernelGGL(components_local_kernel, dim3(g.local_grid), dim3(kLabelRows), 0, stream, mask_in, labels, areas, h, w, g.row_blocks, g.col_blocks, eight, invert);
    if (g.seam_pixels > 0)
        hipLaunchKernelGGL(components_seam_kernel, dim3(g.seam_grid), dim3(kStreamThreads), 0, stream, labels, h, w, g.seam_rows, g.seam_pixels, g.seam_blocks, eight);
    hipLaunchKernelGGL(components_flatten_kernel, dim3(g.flat_grid), dim3(kStreamThreads), 0, stream, labels, areas, h * w, g.flat_blocks, tile_components);
}

static int check_sizes(int64_t n, int64_t h, int64_t w, int connectivity, Grids* g) {
    if (n <= 0) return fail(SX_ERR_BAD_ARG, "n_tiles must be positive, got %lld", (long long)n);
    if (h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "height and width must be positive, got %lld x %lld", (long long)h, (long long)w);
    if (connectivity != 4 && connectivity != 8) return fail(SX_ERR_BAD_ARG, "connectivity must be 4 or 8, got %d", connectivity);
    if (h > 0x7ffffffell / w) return fail(SX_ERR_BAD_ARG, "height x width must not exceed 2^31 - 2 (labels are int32), got %lld x %lld", (long long)h, (long long)w);
    if (!grids_of(n, h, w, g)) return fail(SX_ERR_BAD_ARG, "n_tiles x height x width too large for one call");
    return SX_OK;
}

constexpr size_t kWorkspaceAlign = 256;

}  // namespace components
}  // namespace sx

extern "C" size_t sx_mask_components_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return 8 * (size_t)n * (size_t)h * (size_t)w + sx::components::kWorkspaceAlign;      // labels and areas of sx_mask_area_filter, and room to align them
}

extern "C" int sx_mask_components(const uint8_t* mask_in, int64_t n, int64_t h, int64_t w, int connectivity, int invert, int32_t* labels_out, int32_t* areas_out, unsigned long long* tile_components_out, void* stream_ptr) {
    using namespace sx;
    if (!mask_in) return fail(SX_ERR_BAD_ARG, "mask_in pointer is null");
    if (!labels_out) return fail(SX_ERR_BAD_ARG, "labels_out pointer is null");
    components::Grids g;
    if (int rc = components::check_sizes(n, h, w, connectivity, &g)) return rc;
    if (areas_out == labels_out) return fail(SX_ERR_BAD_ARG, "areas_out must not be labels_out");
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if (tile_components_out && hipMemsetAsync(tile_components_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    components::label_tiles(mask_in, n, h, w, g, connectivity == 8, invert != 0, labels_out, areas_out, tile_components_out, stream);
    return check_launch("mask components");
}

extern "C" int sx_mask_area_filter(const uint8_t* mask_in, uint8_t* mask_out, int64_t n, int64_t h, int64_t w, int connectivity, int holes, int64_t min_area, void* workspace, unsigned long long* tile_counts_out, void* stream_ptr) {
    using namespace sx;
    if (!mask_in) return fail(SX_ERR_BAD_ARG, "mask_in pointer is null");
    if (!mask_out) return fail(SX_ERR_BAD_ARG, "mask_out pointer is null");
    if (!workspace) return fail(SX_ERR_BAD_ARG, "workspace pointer is null");
    components::Grids g;
    if (int rc = components::check_sizes(n, h, w, connectivity, &g)) return rc;
    if (min_area < 1) return fail(SX_ERR_BAD_ARG, "min_area must be at least 1, got %lld", (long long)min_area);
    if (mask_out == mask_in) return fail(SX_ERR_BAD_ARG, "mask_out must not be mask_in: the operation is not in place");
    const uintptr_t ws = reinterpret_cast<uintptr_t>(workspace), out = reinterpret_cast<uintptr_t>(mask_out);
    const size_t pixels = (size_t)n * (size_t)h * (size_t)w;
    if (out < ws + sx_mask_components_workspace_bytes(n, h, w) && ws < out + pixels) return fail(SX_ERR_BAD_ARG, "mask_out must not lie inside the workspace");
    int32_t* labels = reinterpret_cast<int32_t*>((ws + components::kWorkspaceAlign - 1) / components::kWorkspaceAlign * components::kWorkspaceAlign);
    int32_t* areas = labels + pixels;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if (tile_counts_out && hipMemsetAsync(tile_counts_out, 0, sizeof(unsigned long long) * (size_t)n, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    components::label_tiles(mask_in, n, h, w, g, connectivity == 8, holes != 0, labels, areas, nullptr, stream);
    hipLaunchKernelGGL(components::area_filter_kernel, dim3(g.flat_grid), dim3(kStreamThreads), 0, stream, labels, areas, mask_out, (int64_t)h * w, g.flat_blocks, holes != 0, min_area, tile_counts_out);
    return check_launch("mask area filter");
}
