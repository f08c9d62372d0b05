// Elastic deformation with a control grid per tile (sx_elastic_warp / sx_elastic_warp_mask) -- included in macenko.hip right after
// warp.hpp, whose rule it extends at ONE place, the coordinate, and whose functions (warp_effective_row, warp_coord, warp_coord_ok,
// warp_taps) and helpers (blur_to_output, blur_copy, raw_value, store_pack_stream, with_out / with_layout) it uses as they are.
// DESIGN.md 4u.
//
// THE RULE.  Per tile the affine row (a, b, c, d, e, f) of sx_affine_warp AND a control grid (2, GH, GW) of float32 in device memory:
// plane 0 holds dx, plane 1 holds dy, both in SOURCE pixels.  `cell`, an integer 4..SX_ELASTIC_MAX_CELL = 4096, is the control spacing
// in OUTPUT pixels, the same for the whole batch:  GH = (OH - 1) div cell + 4,  GW = (OW - 1) div cell + 4;  control column j sits at
// output column (j - 1) * cell, control row i at output row (i - 1) * cell.  There are n_grids grids, 1 (one for the batch) or N.
//   Displacement  for output pixel (x, y):  jx = x div cell,  tx = float(x - jx * cell) / float(cell)  (one float32 division of two
//            exact floats),  jy and ty likewise.  The uniform cubic B-spline weights of t (elastic_weights), with S = float32(1 / 6):
//              B0 = ((1 - t) (1 - t)) (1 - t) S                         ( (1 - t)^3 / 6 )
//              B1 = fmaf(t t, fmaf(3, t, -6), 4) S                      ( (3 t^3 - 6 t^2 + 4) / 6 )
//              B2 = fmaf(t, fmaf(t, fmaf(-3, t, 3), 3), 1) S            ( (-3 t^3 + 3 t^2 + 3 t + 1) / 6 )
//              B3 = ((t t) t) S                                         ( t^3 / 6 )
//            and the four-term sum (elastic_sum)   sum(w, p) = fmaf(w3, p3, fmaf(w2, p2, fmaf(w1, p1, w0 p0))).
//            The x pass comes first, the y pass second:
//              X_l     = sum(B(tx), P0[jy + l][jx .. jx + 3])     l = 0..3
//              dx(x,y) = sum(B(ty), X_0 .. X_3)                   and dy from plane 1.
//            Everything is float32 with contraction off; every fused multiply-add is written out, ONCE, in the __host__ __device__
//            functions below -- the image kernel, the mask kernel and tools/elastic_index_check.cpp call these very functions.
//   Coordinates   sx = warp_coord(a, b, c, x, y) + dx,  sy = warp_coord(d, e, f, x, y) + dy: one float32 add each.  From there on
//            everything is warp.hpp's rule, unchanged: the limit test (a NaN, an infinite or a huge displacement fails warp_coord_ok:
//            the pixel takes `fill`), the fold, warp_taps, bilinear or nearest, mirror or constant, the output rule, the copy rule.
//   Leave    a row with a NaN or an infinity leaves its tile exactly as in sx_affine_warp (copy, centre crop or centre pad): its grid
//            is NOT read and its displacement is zero.
//   Zero grid  a grid of zeros gives sx_affine_warp's output bit for bit: the weights are finite and >= 0 (t lies in [0, 1): B0 and B3
//            are products of non-negative numbers, B1 and B2 are at least 1 / 6 less a rounding), so every product and every sum of
//            the two passes is a zero, and s + 0.0 is s -- but for s = -0.0, which becomes +0.0: the same floor, the same fraction
//            (0), the same taps.
//   Bounds   NO grid and NO row makes the kernel read outside its tile or its grid.  The tile: warp_taps, as in warp.hpp, whatever
//            float the coordinate is.  The grid: elastic_cell below maps an output column or row to its first control index with the
//            column clamped to OW - 1 (the row to OH - 1) first, so that the columns a ragged block computes past the tile's edge and
//            the rows it stages past OH read indices in [0, GW) and [0, GH) like any other's.  tools/elastic_index_check.cpp sweeps it.
// Five element types, NCHW and NHWC, the three output variants, as sx_affine_warp.  `out` MUST NOT overlap `images`.
//
// THE KERNEL.  ONE launch per call: no workspace, no atomics, no memset.  warp.hpp's geometry: a workgroup of 256 threads takes a
// 32 x 32 output block of one tile, a thread four neighbouring columns of one row; the tile's row is read as uniform words; a tile that
// is left with OH = H and OW = W takes the copy path.  Otherwise the block stages its control points in LDS -- at cell >= 4 a block
// touches at most kElasticSpan = 11 control rows and columns: 2 x 11 x 11 floats --, runs the spline's x pass once per (control row,
// block column) into LDS (2 x 11 x 32 floats: 3.8 KB together, far below what would limit the waves of a CU), and every pixel does its
// four-tap y pass, adds the displacement and goes on as affine_warp_kernel's general path: taps once per pixel, reused for the three
// channels, all loads requested before the first use.  The y weights are one set per thread: its four pixels share the row.
#ifndef SX_ELASTIC_HPP
#define SX_ELASTIC_HPP

#include "warp.hpp"

#ifndef SX_ELASTIC_MIN_CELL
#define SX_ELASTIC_MIN_CELL 4
#define SX_ELASTIC_MAX_CELL 4096
#endif

namespace sx {
namespace elastic_index {

constexpr int kElasticSpan = 11;      // control rows / columns a 32-pixel block touches at cell >= 4: (31 div 4) + 1 + 3
constexpr float kElasticSixth = 1.0f / 6.0f;

// GH of OH (GW of OW): the control points an axis of `on` output pixels reads.
__host__ __device__ inline int64_t elastic_grid_dim(int64_t on, int cell) { return (on - 1) / cell + 4; }

// An output column (row) x >= 0 of an axis of `on` pixels -> j, the first of the four control indices j .. j + 3 it reads, and t in
// [0, 1).  x is clamped to on - 1 first: j + 3 <= (on - 1) div cell + 3 = elastic_grid_dim(on, cell) - 1 whatever x is.
__host__ __device__ inline int elastic_cell(int64_t x, int64_t on, int cell, float& t) {
    const uint32_t xc = (uint32_t)(x < on ? x : on - 1);      // (on < 2^32: the call checks it)
    const uint32_t j = xc / (uint32_t)cell;
    t = (float)(xc - j * (uint32_t)cell) / (float)cell;
    return (int)j;
}

__host__ __device__ inline void elastic_weights(float t, float (&w)[4]) {
#pragma clang fp contract(off)
    const float u = 1.0f - t;
    w[0] = ((u * u) * u) * kElasticSixth;
    w[1] = fmaf(t * t, fmaf(3.0f, t, -6.0f), 4.0f) * kElasticSixth;
    w[2] = fmaf(t, fmaf(t, fmaf(-3.0f, t, 3.0f), 3.0f), 1.0f) * kElasticSixth;
    w[3] = ((t * t) * t) * kElasticSixth;
}

__host__ __device__ inline float elastic_sum(const float (&w)[4], float p0, float p1, float p2, float p3) {
#pragma clang fp contract(off)
    return fmaf(w[3], p3, fmaf(w[2], p2, fmaf(w[1], p1, w[0] * p0)));
}

// The control rows (columns) a block that starts at output row (column) `start` stages: the first index and how many, at most
// kElasticSpan.  The block's last pixel is start + side - 1, clamped like any other.
__host__ __device__ inline int elastic_block_span(int64_t start, int side, int64_t on, int cell, int& first) {
    float unused;
    first = elastic_cell(start, on, cell, unused);
    const int count = elastic_cell(start + side - 1, on, cell, unused) - first + 4;
    return count < kElasticSpan ? count : kElasticSpan;
}

// A pixel's or a staged column's position inside the block's staged span: j - first, never past kElasticSpan - 4 (it is not: the
// span of a block holds all its pixels' indices -- the host check asserts that; the clamp keeps a reader of this line from having to).
__host__ __device__ inline int elastic_local(int j, int first) {
    const int at = j - first;
    return at < kElasticSpan - 4 ? at : kElasticSpan - 4;
}

}  // namespace elastic_index
}  // namespace sx

#ifndef SX_WARP_INDEX_ONLY
namespace sx {
namespace macenko {

using namespace elastic_index;

struct ElasticArgs {
    const float* grids;              // n_grids x 2 x GH x GW floats
    int64_t grid_height, grid_width;
    int per_grid;                    // 1: grid `tile`, 0: one grid for the batch
    int cell;
};

// kPlanes = 3: the tiles; kPlanes = 1 (uint8, planar, nearest): the masks.
template <typename T, typename O, bool kUnit, bool kInter, int kPlanes>
__global__ __launch_bounds__(kWarpThreads) void elastic_warp_kernel(const T* __restrict__ images, O* __restrict__ out, const WarpArgs a, const ElasticArgs g) {
#pragma clang fp contract(off)      // (every fused multiply-add is written out)
    static_assert(!(kInter && kPlanes == 1), "a mask is one plane");
    __shared__ float control[2][kElasticSpan][kElasticSpan];      // the block's control points
    __shared__ float across[2][kElasticSpan][kWarpSide];          // the x pass: per plane, control row and block column
    const int tid = threadIdx.x;
    const int per_tile = a.row_blocks * a.col_blocks;
    const int64_t tile = blockIdx.x / (unsigned)per_tile;
    const int within = (int)(blockIdx.x % (unsigned)per_tile);
    const int64_t y0 = (int64_t)(within / a.col_blocks) * kWarpSide, x0 = (int64_t)(within % a.col_blocks) * kWarpSide;
    const int64_t height = a.height, width = a.width, pixels = height * width;
    const int64_t out_height = a.out_height, out_width = a.out_width, out_pixels = out_height * out_width;
    const T* img = images + tile * kPlanes * pixels;
    O* dst = out + tile * kPlanes * out_pixels;
    const int rows_in = (int)min((int64_t)kWarpSide, out_height - y0), cols_in = (int)min((int64_t)kWarpSide, out_width - x0);      // the block inside the output tile

    auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    float given[6], row[6];
    const float* from = a.rows + (a.per_row ? tile * 6 : 0);
#pragma unroll
    for (int k = 0; k < 6; ++k) given[k] = uniform(from[k]);
    const bool anchor = warp_effective_row(given, height, width, out_height, out_width, row);      // (the same for every thread of the block)

    if (anchor && height == out_height && width == out_width) {      // ---- a copy tile: affine_warp_kernel's copy path; the grid is not read
        const int lines = kInter ? rows_in : kPlanes * rows_in, length = kInter ? 3 * cols_in : cols_in;
        auto line_start = [&](int line) -> int64_t {
            if constexpr (kInter) return ((y0 + line) * width + x0) * 3; else return (int64_t)(line / rows_in) * pixels + (y0 + line % rows_in) * width + x0;
        };
        if (a.vec_copy) {      // (width % 4 == 0: every line starts on a pack and is a whole number of packs)
            const int packs = length / 4;
            for (int i = tid; i < lines * packs; i += kWarpThreads) {
                const int64_t at = line_start(i / packs) + 4 * (i % packs);
                const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(img + at);
                O res[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) res[e] = blur_copy<T, O, kUnit>(pk.v[e]);
                store_pack_stream<O, 4>(dst + at, res);
            }
        } else {
            for (int i = tid; i < lines * length; i += kWarpThreads) {
                const int64_t at = line_start(i / length) + i % length;
                dst[at] = blur_copy<T, O, kUnit>(img[at]);
            }
        }
        return;
    }

    // ---- the displacement: control points -> LDS, the x pass -> LDS (a tile that is left has none: its grid is not read)
    const int cell = g.cell;
    int first_row = 0, first_col = 0;
    if (!anchor) {
        const int64_t grid_height = g.grid_height, grid_width = g.grid_width;
        const int n_rows = elastic_block_span(y0, kWarpSide, out_height, cell, first_row), n_cols = elastic_block_span(x0, kWarpSide, out_width, cell, first_col);
        const float* grid = g.grids + (g.per_grid ? tile * 2 * grid_height * grid_width : 0);
        for (int i = tid; i < 2 * n_rows * n_cols; i += kWarpThreads) {      // (first + n <= GH, GW: elastic_cell's clamp)
            const int plane = i / (n_rows * n_cols), rest = i % (n_rows * n_cols), r = rest / n_cols, c = rest % n_cols;
            control[plane][r][c] = grid[(plane * grid_height + first_row + r) * grid_width + first_col + c];
        }
        __syncthreads();
        for (int i = tid; i < 2 * n_rows * kWarpSide; i += kWarpThreads) {
            const int col = i % kWarpSide, line = i / kWarpSide, r = line % n_rows, plane = line / n_rows;
            float t, w[4];
            const int j = elastic_local(elastic_cell(x0 + col, out_width, cell, t), first_col);
            elastic_weights(t, w);
            const float* p = control[plane][r];
            across[plane][r][col] = elastic_sum(w, p[j], p[j + 1], p[j + 2], p[j + 3]);
        }
        __syncthreads();
    }

    // ---- the general path: a thread's row and its four columns
    const int r = tid / kWarpGroups, col0 = 4 * (tid % kWarpGroups);
    const int64_t gy = y0 + r, gx = x0 + col0;
    if (r >= rows_in || gx >= out_width) return;
    const bool nearest = a.nearest != 0, constant = a.constant != 0;
    const float fill = a.fill;
    const O fill_out = blur_to_output<T, O, kUnit>(fill);
    const float yf = (float)gy;
    float dxs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dys[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!anchor) {
        float t, w[4];
        const int j = elastic_local(elastic_cell(gy, out_height, cell, t), first_row);
        elastic_weights(t, w);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            dxs[p] = elastic_sum(w, across[0][j][col0 + p], across[0][j + 1][col0 + p], across[0][j + 2][col0 + p], across[0][j + 3][col0 + p]);
            dys[p] = elastic_sum(w, across[1][j][col0 + p], across[1][j + 1][col0 + p], across[1][j + 2][col0 + p], across[1][j + 3][col0 + p]);
        }
    }
    WarpTaps taps[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {      // (a column past the tile's edge is computed and not stored: its indices are inside the tile and the grid like any other's)
        const float xf = (float)(gx + p);
        taps[p] = warp_taps(warp_coord(row[0], row[1], row[2], xf, yf) + dxs[p], warp_coord(row[3], row[4], row[5], xf, yf) + dys[p], nearest, constant, height, width);
    }
    const int64_t step = kInter ? 3 : 1;
    const int64_t first = gy * out_width + gx;      // the first of the four output pixels
#pragma unroll
    for (int c = 0; c < kPlanes; ++c) {
        const T* plane = img + (kInter ? (int64_t)c : c * pixels);
        O res[4];
        if (nearest) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const T v = plane[(int64_t)taps[p].at[0] * step];
                res[p] = (taps[p].outside & 1u) ? fill_out : blur_copy<T, O, kUnit>(v);
            }
        } else {
            T v[4][4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int k = 0; k < 4; ++k) v[p][k] = plane[(int64_t)taps[p].at[k] * step];      // (all sixteen requested before the first is used)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float f[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) f[k] = ((taps[p].outside >> k) & 1u) ? fill : raw_value<T>(v[p][k]);
                const float fx = taps[p].fx, fy = taps[p].fy;
                const float top = fmaf(fx, f[1] - f[0], f[0]);
                const float bot = fmaf(fx, f[3] - f[2], f[2]);
                res[p] = blur_to_output<T, O, kUnit>(fmaf(fy, bot - top, top));
                if (fx == 0.0f && fy == 0.0f) res[p] = (taps[p].outside & 1u) ? fill_out : blur_copy<T, O, kUnit>(v[p][0]);      // the stored element, no arithmetic
            }
        }
        if (a.vec_out) {      // (out_width % 4 == 0: the four columns are inside the tile)
            store_pack_stream<O, 4>(dst + c * out_pixels + first, res);
        } else {
            O* to = dst + (kInter ? (int64_t)c : c * out_pixels);
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (gx + p < out_width) to[(first + p) * step] = res[p];
        }
    }
}

template <typename T, typename O, bool kUnit, bool kInter, int kPlanes>
static int elastic_warp_launch(const void* images, void* out, WarpArgs a, const ElasticArgs& g, bool quads_in, bool quads_out, hipStream_t stream) {
    a.vec_out = quads_out && !kInter;
    a.vec_copy = quads_in && quads_out;
    const unsigned grid = (unsigned)(a.n_tiles * a.row_blocks * a.col_blocks);
    hipLaunchKernelGGL((elastic_warp_kernel<T, O, kUnit, kInter, kPlanes>), dim3(grid), dim3(kWarpThreads), 0, stream, static_cast<const T*>(images), static_cast<O*>(out), a, g);
    return check_launch("elastic warp");
}

template <typename T>
static int elastic_warp_typed(const void* images, void* out, const WarpArgs& a, const ElasticArgs& g, int out_code, bool interleaved, bool unit, hipStream_t stream) {
    const bool quads_in = a.width % 4 == 0 && aligned_for(images, 4 * sizeof(T));
    const bool quads_out = a.out_width % 4 == 0 && aligned_for(out, 4 * out_elem_bytes(sizeof(T), out_code, unit));
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<1>(false, interleaved, [&](auto, auto inter) {
            return elastic_warp_launch<T, O, decltype(u)::value, decltype(inter)::value, 3>(images, out, a, g, quads_in, quads_out, stream);
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
// affine_warp_common's checks, in its order and words, then the grid's; everything returns before anything is enqueued.
static int elastic_warp_common(const void* images, const void* out, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows, const float* grids,
                               int64_t n_grids, int cell, int interpolation, int border, sx::macenko::WarpArgs& a, sx::macenko::ElasticArgs& g) {
    int rc = affine_warp_common(images, out, n, h, w, oh, ow, rows, n_rows, interpolation, border, a);
    if (rc != SX_OK) return rc;
    if (!grids) return fail(SX_ERR_BAD_ARG, "grids pointer is null");
    if ((rc = check_rows("n_grids", n_grids, n)) != SX_OK) return rc;
    if (cell < SX_ELASTIC_MIN_CELL || cell > SX_ELASTIC_MAX_CELL)
        return fail(SX_ERR_BAD_ARG, "cell must lie in SX_ELASTIC_MIN_CELL (%d) .. SX_ELASTIC_MAX_CELL (%d), got %d", SX_ELASTIC_MIN_CELL, SX_ELASTIC_MAX_CELL, cell);
    g.grids = grids;
    g.grid_height = sx::elastic_index::elastic_grid_dim(oh, cell);
    g.grid_width = sx::elastic_index::elastic_grid_dim(ow, cell);
    g.per_grid = rows_per_tile(n_grids, n);
    g.cell = cell;
    return SX_OK;
}

extern "C" int sx_elastic_warp(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows, const float* grids,
                               int64_t n_grids, int cell, int interpolation, int border, float fill, unsigned flags, void* stream_ptr) {
    sx::macenko::WarpArgs a{};
    sx::macenko::ElasticArgs g{};
    int rc = elastic_warp_common(images, out, n, h, w, oh, ow, rows, n_rows, grids, n_grids, cell, interpolation, border, a, g);
    if (rc != SX_OK) return rc;
    if (!(std::fabs(fill) < __builtin_huge_valf())) return fail(SX_ERR_BAD_ARG, "fill must be finite, got %g", (double)fill);
    rc = deconv_flags_ok(flags, dtype, false, "sx_elastic_warp");
    if (rc != SX_OK) return rc;
    a.fill = dtype == SX_U8 ? std::fmin(std::fmax(fill, 0.0f), 255.0f) : fill;      // (a level: the output rule's cast takes 0..255)
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return elastic_warp_typed<typename decltype(t)::type>(images, out, a, g, out_code, inter, unit, stream); });
}

extern "C" int sx_elastic_warp_mask(const unsigned char* mask, unsigned char* out, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows,
                                    const float* grids, int64_t n_grids, int cell, int border, int fill, void* stream_ptr) {
    sx::macenko::WarpArgs a{};
    sx::macenko::ElasticArgs g{};
    int rc = elastic_warp_common(mask, out, n, h, w, oh, ow, rows, n_rows, grids, n_grids, cell, SX_WARP_NEAREST, border, a, g);
    if (rc != SX_OK) return rc;
    if (fill < 0 || fill > 255) return fail(SX_ERR_BAD_ARG, "fill must be a byte 0..255, got %d", fill);
    a.fill = (float)fill;
    const bool quads_in = w % 4 == 0 && aligned_for(mask, 4), quads_out = ow % 4 == 0 && aligned_for(out, 4);
    return elastic_warp_launch<uint8_t, uint8_t, false, false, 1>(mask, out, a, g, quads_in, quads_out, static_cast<hipStream_t>(stream_ptr));
}
#endif  // SX_WARP_INDEX_ONLY
#endif  // SX_ELASTIC_HPP
