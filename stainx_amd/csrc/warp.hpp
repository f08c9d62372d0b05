// Affine warp with a row per tile (sx_affine_warp / sx_affine_warp_mask) -- included at the end of macenko.hip next to blur.hpp, whose
// helpers it uses as they are: blur_to_output, blur_copy, raw_value, store_pack_stream, with_out / with_layout.  DESIGN.md 4t.
//
// THE RULE.  Per tile ONE row of six float32 (a, b, c, d, e, f) is read from device memory.  The row maps an OUTPUT pixel to the SOURCE
// position, in pixel-index coordinates with pixel centres at integers (scipy.ndimage.affine_transform, cv2.warpAffine with
// WARP_INVERSE_MAP, grid_sample(align_corners=True) after un-normalising).  The source tile is H x W, the output tile OH x OW: crop, pad
// and resize are the same call.  For output column x and row y
//            sx = fmaf(a, x, fmaf(b, y, c))      sy = fmaf(d, x, fmaf(e, y, f))      (float32; x and y are exact as floats)
//   Anchor   a row with a NaN or an infinity means "leave this tile": it is replaced by (1, 0, (W - OW) div 2, 0, 1, (H - OH) div 2),
//            floor division.  OH = H and OW = W: a copy; otherwise the centre crop, or the centre pad by the border rule.
//   Limit    a coordinate that is not finite or whose magnitude exceeds SX_WARP_MAX_COORD = 2^22 makes the pixel take `fill`, in both
//            border modes.  This is tested in float32 BEFORE any conversion to an integer: every integer below is at most 2^22 + 1 in
//            magnitude.  The rows live on the device and may hold anything; NO value of a row produces a tap index outside the tile
//            (warp_taps below returns positions inside the plane whatever floats it is given; tools/warp_index_check.cpp sweeps it).
//   Borders  SX_WARP_MIRROR reflects WITHOUT repeating the edge, inside the pixel's own tile, folded as often as needed: period
//            2 (n - 1), an axis of length 1 maps to 0 -- blur.hpp's and focus.hpp's fold, scipy's mode="mirror", torch's "reflection"
//            with align_corners=True.  SX_WARP_CONSTANT: a tap outside the tile is `fill` (scipy's "grid-constant", cv2's
//            BORDER_CONSTANT, grid_sample's "zeros" at fill = 0).  `fill` is a float32 on the element's own scale -- a level for uint8
//            tiles (clamped to 0..255 by the call), taken as it is for float tiles -- and goes through the output rule.
//   Bilinear x0 = floorf(sx), fx = sx - x0 (exact, but for a negative sx tinier than 2^-25, where it rounds to 1), y0 and fy likewise; the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1),
//            each through the border rule, as the element type stores them (a uint8 byte is its level, a float element as it is):
//            top = fmaf(fx, v01 - v00, v00);  bot = fmaf(fx, v11 - v10, v10);  v = fmaf(fy, bot - top, top).
//            Each step lies between its operands: nothing is clamped.  fx == 0 and fy == 0: the pixel is the stored element through
//            the copy rule, no arithmetic touches it.  Non-finite pixels are not special.
//   Nearest  xi = floorf(sx + 0.5f), yi likewise, in float32 (scipy's order=0); the stored element at (xi, yi) through the border rule
//            and the copy rule.  (It IS the bilinear rule at the rounded coordinates: fx = fy = 0.)
//   Output   blur.hpp's: blur_to_output (an 8-bit level ROUNDED to nearest, SX_MACENKO_OUT_BF16 / _OUT_F16 for uint8 tiles, the / 255 of
//            SX_MACENKO_NORMALIZE_0_1) and, for copied elements, blur_copy (the input's bits where the output element is the input
//            element and nothing is divided: NaN payloads and -0.0 included).
//   Masks    a mask does not select pixels here; it is warped WITH its tile by sx_affine_warp_mask: one uint8 plane per tile, nearest,
//            bytes moved as bytes (labels 0..255 survive), mirror or constant with a fill byte.
// Five element types, NCHW and NHWC.  `out` MUST NOT overlap `images`: a workgroup reads source pixels other workgroups' outputs would
// overwrite.
//
// THE KERNEL.  ONE launch per call: no workspace, no atomics, no memset, no LDS.  A workgroup of 256 threads takes a 32 x 32 output
// block of one tile; a thread takes four neighbouring output columns of one row, so a WAVE covers 32 columns x 8 rows -- roughly square,
// and a rotation by any angle touches about the same number of source lines.  A wave reads its tile's six floats as uniform words
// (readfirstlane) and decides the tile's path once:
//   copy     an anchor row with OH = H and OW = W: the block is streamed through with packs, as blur.hpp's copy path.
//   general  coordinates, weights and the four folded tap offsets are computed ONCE per pixel and reused for the three channels.  The
//            taps are single-element global loads through the vector cache (a gather); planar outputs are written as 4-pixel packs
//            where aligned, single elements otherwise and for NHWC.  Interpolation and border are wave-uniform run-time branches.
#ifndef SX_WARP_HPP
#define SX_WARP_HPP

#include <cmath>
#include <cstdint>

#ifndef __HIPCC__      // (tools/warp_index_check.cpp compiles the index arithmetic for the host alone)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#ifndef SX_WARP_MAX_COORD
#define SX_WARP_MAX_COORD 4194304.0f
#endif

namespace sx {
namespace warp_index {

constexpr float kWarpMaxCoord = SX_WARP_MAX_COORD;      // 2^22: a coordinate within it has an exact floor, an exact fraction, and fits an int with room for + 1
constexpr int kWarpFoldDirect = 1 << 23;                  // an axis longer than this is never left twice by an index within the limit

// (W - OW) div 2 and (H - OH) div 2 with floor division, as floats.
__host__ __device__ inline float warp_anchor_offset(int64_t n, int64_t on) {
    const int64_t d = n - on;
    return (float)(d >= 0 ? d / 2 : -((1 - d) / 2));
}

// The row a tile uses: its own, or the anchor row where one of the six is a NaN or an infinity.  -> was it replaced?
__host__ __device__ inline bool warp_effective_row(const float (&row)[6], int64_t h, int64_t w, int64_t oh, int64_t ow, float (&use)[6]) {
    bool finite = true;
    for (int k = 0; k < 6; ++k) {
        finite = finite && fabsf(row[k]) < __builtin_huge_valf();      // (false for a NaN)
        use[k] = row[k];
    }
    if (!finite) {
        use[0] = 1.0f, use[1] = 0.0f, use[2] = warp_anchor_offset(w, ow);
        use[3] = 0.0f, use[4] = 1.0f, use[5] = warp_anchor_offset(h, oh);
    }
    return !finite;
}

__host__ __device__ inline float warp_coord(float a, float b, float c, float x, float y) { return fmaf(a, x, fmaf(b, y, c)); }

// A coordinate the rule goes on with: finite and within the limit (false for a NaN).
__host__ __device__ inline bool warp_coord_ok(float s) { return fabsf(s) <= kWarpMaxCoord; }

// q reflected into 0..n-1 without repeating the edge; |q| <= 2^22 + 1, n >= 1.
__host__ __device__ inline int warp_fold(int q, int64_t n) {
    if (q >= 0 && q < n) return q;
    if (n == 1) return 0;
    if (n > kWarpFoldDirect) return -q;      // (q < 0 here: q < 2^23 < n; one reflection at 0 and -q < n)
    const int period = 2 * ((int)n - 1);
    int m = q % period;
    m = m < 0 ? m + period : m;
    return m >= (int)n ? period - m : m;
}

// One axis of a pixel: the coordinate s -- warp_coord_ok(s) holds: warp_taps has tested it -- -> the indices of its two taps, each in [0, n), the fraction, and which of the
// two lie outside the tile under the constant border (bit 0: the first, bit 1: the second; their index is 0 then).
__host__ __device__ inline float warp_axis(float s, bool constant, int64_t n, int (&index)[2], unsigned& outside) {
    const float s0 = floorf(s);
    const int q0 = (int)s0;      // |s0| <= 2^22
    outside = 0u;
    for (int k = 0; k < 2; ++k) {
        const int q = q0 + k;
        if (constant) {
            const bool in = q >= 0 && q < n;
            index[k] = in ? q : 0;
            outside |= in ? 0u : 1u << k;
        } else {
            index[k] = warp_fold(q, n);
        }
    }
    return s - s0;
}

// A pixel's four taps: their positions in the H x W plane (y * W + x, below H * W < 2^32), its two fractions and which taps take `fill`
// (bit 0: (x0, y0), bit 1: (x0 + 1, y0), bit 2: (x0, y0 + 1), bit 3: (x0 + 1, y0 + 1)).  A pixel whose coordinates fail the limit has
// fx = fy = 0, all four bits set and positions 0.
struct WarpTaps {
    uint32_t at[4];
    float fx, fy;
    unsigned outside;
};

__host__ __device__ inline WarpTaps warp_taps(float sx, float sy, bool nearest, bool constant, int64_t h, int64_t w) {
    WarpTaps t;
    t.at[0] = t.at[1] = t.at[2] = t.at[3] = 0u;
    t.fx = t.fy = 0.0f;
    t.outside = 0xFu;
    if (!(warp_coord_ok(sx) && warp_coord_ok(sy))) return t;
    if (nearest) {      // (within the limit s + 0.5 is exact or a tie of the addition, and its floor is at most 2^22)
        sx = floorf(sx + 0.5f);
        sy = floorf(sy + 0.5f);
    }
    int xs[2], ys[2];
    unsigned out_x, out_y;
    t.fx = warp_axis(sx, constant, w, xs, out_x);
    t.fy = warp_axis(sy, constant, h, ys, out_y);
    t.outside = 0u;
    for (int k = 0; k < 4; ++k) {
        const bool out = (((out_x >> (k & 1)) | (out_y >> (k >> 1))) & 1u) != 0u;
        t.outside |= out ? 1u << k : 0u;
        t.at[k] = out ? 0u : (uint32_t)((int64_t)ys[k >> 1] * w + xs[k & 1]);
    }
    return t;
}

}  // namespace warp_index
}  // namespace sx

#ifndef SX_WARP_INDEX_ONLY
namespace sx {
namespace macenko {

using namespace warp_index;

constexpr int kWarpSide = 32;            // the output block
constexpr int kWarpThreads = 256;
constexpr int kWarpGroups = kWarpSide / 4;      // threads per row of the block: a wave is 8 of them x 8 rows

struct WarpArgs {
    const float* rows;               // n_rows x 6 floats
    int64_t height, width;           // the source tile
    int64_t out_height, out_width;   // the output tile
    int64_t n_tiles;
    int row_blocks, col_blocks;      // workgroups per tile
    int per_row;                     // 1: row `tile`, 0: one row for the batch
    int nearest, constant;           // interpolation and border: uniform branches
    float fill;
    int vec_out;                     // planar: 4-pixel packs of the output
    int vec_copy;                    // the copy path's packs (either layout)
};

// kPlanes = 3: the tiles; kPlanes = 1 (uint8, planar, nearest): the masks.
template <typename T, typename O, bool kUnit, bool kInter, int kPlanes>
__global__ __launch_bounds__(kWarpThreads) void affine_warp_kernel(const T* __restrict__ images, O* __restrict__ out, WarpArgs a) {
#pragma clang fp contract(off)      // (every fused multiply-add is written out)
    static_assert(!(kInter && kPlanes == 1), "a mask is one plane");
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
    const bool anchor = warp_effective_row(given, height, width, out_height, out_width, row);

    if (anchor && height == out_height && width == out_width) {      // ---- a copy tile: the block's elements streamed through (blur.hpp's copy path)
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

    // ---- the general path: a thread's row and its four columns
    const int r = tid / kWarpGroups;
    const int64_t gy = y0 + r, gx = x0 + 4 * (tid % kWarpGroups);
    if (r >= rows_in || gx >= out_width) return;
    const bool nearest = a.nearest != 0, constant = a.constant != 0;
    const float fill = a.fill;
    const O fill_out = blur_to_output<T, O, kUnit>(fill);
    const float yf = (float)gy;
    const float along_x = fmaf(row[1], yf, row[2]), along_y = fmaf(row[4], yf, row[5]);      // fmaf(b, y, c) and fmaf(e, y, f): the same for the four
    WarpTaps taps[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {      // (a column past the tile's edge is computed and not stored: its indices are inside the tile like any other's)
        const float xf = (float)(gx + p);
        taps[p] = warp_taps(fmaf(row[0], xf, along_x), fmaf(row[3], xf, along_y), nearest, constant, height, width);
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
static int affine_warp_launch(const void* images, void* out, WarpArgs a, bool quads_in, bool quads_out, hipStream_t stream) {
    a.vec_out = quads_out && !kInter;
    a.vec_copy = quads_in && quads_out;
    const unsigned grid = (unsigned)(a.n_tiles * a.row_blocks * a.col_blocks);
    hipLaunchKernelGGL((affine_warp_kernel<T, O, kUnit, kInter, kPlanes>), dim3(grid), dim3(kWarpThreads), 0, stream, static_cast<const T*>(images), static_cast<O*>(out), a);
    return check_launch("affine warp");
}

template <typename T>
static int affine_warp_typed(const void* images, void* out, const WarpArgs& a, int out_code, bool interleaved, bool unit, hipStream_t stream) {
    const bool quads_in = a.width % 4 == 0 && aligned_for(images, 4 * sizeof(T));
    const bool quads_out = a.out_width % 4 == 0 && aligned_for(out, 4 * out_elem_bytes(sizeof(T), out_code, unit));
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<1>(false, interleaved, [&](auto, auto inter) {
            return affine_warp_launch<T, O, decltype(u)::value, decltype(inter)::value, 3>(images, out, a, quads_in, quads_out, stream);
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
// The checks both calls share, in the sibling calls' order and words; everything returns before anything is enqueued.
static int affine_warp_common(const void* images, const void* out, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows, int interpolation,
                              int border, sx::macenko::WarpArgs& a) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    int rc = check_tiles(n, h, w);
    if (rc != SX_OK) return rc;
    if (oh <= 0 || ow <= 0) return fail(SX_ERR_BAD_ARG, "the output tile must have positive sizes, got OH=%lld OW=%lld", (long long)oh, (long long)ow);
    if (oh >= (1ll << 32) || ow >= (1ll << 32) || oh * ow >= (1ll << 32) || n * oh * ow >= (1ll << 32)) return fail(SX_ERR_BAD_ARG, "N*OH*OW must be below 2^32 pixels");
    if (!rows) return fail(SX_ERR_BAD_ARG, "rows pointer is null");
    if ((rc = check_rows("n_rows", n_rows, n)) != SX_OK) return rc;
    if (interpolation != SX_WARP_NEAREST && interpolation != SX_WARP_BILINEAR)
        return fail(SX_ERR_BAD_ARG, "interpolation must be SX_WARP_NEAREST (0) or SX_WARP_BILINEAR (1), got %d", interpolation);
    if (border != SX_WARP_MIRROR && border != SX_WARP_CONSTANT) return fail(SX_ERR_BAD_ARG, "border must be SX_WARP_MIRROR (0) or SX_WARP_CONSTANT (1), got %d", border);
    const int64_t row_blocks = (oh + sx::macenko::kWarpSide - 1) / sx::macenko::kWarpSide, col_blocks = (ow + sx::macenko::kWarpSide - 1) / sx::macenko::kWarpSide;
    if (n * row_blocks * col_blocks > 0x7fffffffll) return fail(SX_ERR_BAD_ARG, "images too large for one call");      // (n * oh * ow < 2^32: each factor fits an int)
    a.rows = rows;
    a.height = h;
    a.width = w;
    a.out_height = oh;
    a.out_width = ow;
    a.n_tiles = n;
    a.row_blocks = (int)row_blocks;
    a.col_blocks = (int)col_blocks;
    a.per_row = rows_per_tile(n_rows, n);
    a.nearest = interpolation == SX_WARP_NEAREST;
    a.constant = border == SX_WARP_CONSTANT;
    return SX_OK;
}

extern "C" int sx_affine_warp(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows, int interpolation,
                              int border, float fill, unsigned flags, void* stream_ptr) {
    sx::macenko::WarpArgs a{};
    int rc = affine_warp_common(images, out, n, h, w, oh, ow, rows, n_rows, interpolation, border, a);
    if (rc != SX_OK) return rc;
    if (!(std::fabs(fill) < __builtin_huge_valf())) return fail(SX_ERR_BAD_ARG, "fill must be finite, got %g", (double)fill);
    rc = deconv_flags_ok(flags, dtype, false, "sx_affine_warp");
    if (rc != SX_OK) return rc;
    a.fill = dtype == SX_U8 ? std::fmin(std::fmax(fill, 0.0f), 255.0f) : fill;      // (a level: the output rule's cast takes 0..255)
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return affine_warp_typed<typename decltype(t)::type>(images, out, a, out_code, inter, unit, stream); });
}

extern "C" int sx_affine_warp_mask(const unsigned char* mask, unsigned char* out, int64_t n, int64_t h, int64_t w, int64_t oh, int64_t ow, const float* rows, int64_t n_rows, int border,
                                   int fill, void* stream_ptr) {
    sx::macenko::WarpArgs a{};
    int rc = affine_warp_common(mask, out, n, h, w, oh, ow, rows, n_rows, SX_WARP_NEAREST, border, a);
    if (rc != SX_OK) return rc;
    if (fill < 0 || fill > 255) return fail(SX_ERR_BAD_ARG, "fill must be a byte 0..255, got %d", fill);
    a.fill = (float)fill;
    const bool quads_in = w % 4 == 0 && aligned_for(mask, 4), quads_out = ow % 4 == 0 && aligned_for(out, 4);
    return affine_warp_launch<uint8_t, uint8_t, false, false, 1>(mask, out, a, quads_in, quads_out, static_cast<hipStream_t>(stream_ptr));
}
#endif  // SX_WARP_INDEX_ONLY
#endif  // SX_WARP_HPP
