// JPEG compression round trip with a quality per tile (sx_jpeg_roundtrip / sx_jpeg_roundtrip_masked) -- included at the end of macenko.hip
// next to blur.hpp, whose helpers it uses as they are: raw_value, hsv_to_output, MaskArgs / tile_mask, Pack, store_pack_stream, with_out /
// with_layout.  DESIGN.md 4w.
//
// THE RULE is stated in include/stainx_hip.h: what baseline JPEG (libjpeg's integer "islow" path) at the tile's quality decodes to, bit for
// bit, with no bitstream in between -- the entropy coder is lossless.  Its arithmetic is jpeg_block.hpp, int32 throughout; this file is the
// data movement.
//   Input    a uint8 byte is its level; a float element x (converted to float32 first) is clamp(rint(255 x), 0, 255), a NaN is level 0.
//            The codec sees 8-bit levels: this quantisation is part of the feature.
//   Output   the decoded 8-bit level through the output rule of sx_hsv_apply (hsv_to_output: an integer, nothing is rounded).
//   Copies   a tile whose quality is NaN, infinite or < 1 and -- masked call -- a masked-out pixel: sx_hsv_apply's copy, the input level
//            clamped to [0, 255] through the output rule (uint8 in, uint8 out: the same bytes).
//
// THE KERNEL.  ONE launch per call: no workspace, no atomics, no memset, nothing through device memory between encode and decode.  A
// workgroup of 256 threads owns a region of one tile aligned to 16 pixels -- 128 x 64 in 4:4:4, 128 x 128 in 4:2:0 -- and keeps its planes
// in LDS as BYTES (every stage of the codec hands 8-bit levels to the next):
//   0. tables   the tile's quality (every lane the same word, then readfirstlane); 128 threads compute one table entry and its reciprocal
//               multiplier each.  A copy tile streams its region through and leaves.
//   1. colour   a thread takes 4 neighbouring pixels of a row (aligned planar input: one pack per channel), converts them and stores 4 Y
//               bytes -- in 4:4:4 also 4 Cb and 4 Cr bytes -- as one word; rows and columns past the tile's edge replicate the last pixel up
//               to whole blocks.  4:2:0: a second sweep over the chroma WINDOW, the region's 64 x 64 chroma samples with one block (8
//               samples) of halo on each side, 80 x 80: a thread takes 2 x 4 pixels, and stores two Cb and two Cr means.
//   2. blocks   ONE THREAD PER 8 x 8 BLOCK: it reads the block's 64 bytes (eight 8-byte words), runs the forward DCT, the quantiser, the
//               dequantiser and the inverse DCT in registers and writes the 64 decoded bytes back over the block.  No thread reads another's
//               block: no barrier inside the codec.  4:4:4: 384 blocks, 4:2:0: 256 + 2 x 100.
//   3. output   a thread takes 4 neighbouring pixels of a row: Y, the chroma (4:2:0: the triangle filter on the window, which holds the one
//               sample beyond the region that the filter reads on each side), RGB, the output rule, one pack per channel or single elements.
// In 4:2:0 the 36 halo blocks of each chroma plane are decoded again by the neighbouring workgroups: recomputation, not communication.
// 456 blocks are coded where 384 would do (256 luma + 2 x 64): 19 % more block work, and the chroma sweep loads (160 / 128)^2 = 1.56 x the
// region's pixels.  LDS: 31 232 bytes of planes + 768 of tables.
namespace sx {
namespace macenko {

namespace jb = sx::jpeg_block;

constexpr int kJpegThreads = 256;

struct JpegArgs {
    const float* qualities;       // n_rows floats
    int64_t height, width, n_tiles;
    int row_regions, col_regions; // workgroups per tile
    int per_row;                  // 1: quality `tile`, 0: one quality for the batch
    int sub;                      // 0: 4:4:4, 2: 4:2:0
    int vec_in, vec_out;          // planar: 4-pixel packs of the input / of the output
    int vec_copy;                 // the copy path's packs (either layout)
    int mask_vec;                 // the mask's four bytes as one word
};

template <typename T> __device__ __forceinline__ int jpeg_level_of(T v) {
    if constexpr (sizeof(T) == 1) return (int)v; else return jb::jpeg_level(raw_value<T>(v));
}

// sx_hsv_apply's copy of an element: the input level, clamped, through the output rule.
template <typename T, typename O, bool kUnit>
__device__ __forceinline__ O jpeg_copy(T v) {
#pragma clang fp contract(off)
    float level;
    if constexpr (sizeof(T) == 1) level = (float)v; else level = fminf(fmaxf(raw_value<T>(v) * 255.0f, 0.0f), 255.0f);
    return hsv_to_output<T, O, kUnit>(level);
}

template <typename T, typename O, bool kUnit, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kJpegThreads) void jpeg_roundtrip_kernel(const T* __restrict__ images, O* __restrict__ out, JpegArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    static_assert(!(kInter && kMask), "the masked forms are planar");
    __shared__ __attribute__((aligned(16))) uint8_t planes[jb::kJpegPlaneBytes];
    __shared__ uint16_t table_q[128];      // luminance, then chrominance
    __shared__ uint32_t table_m[128];
    const int tid = threadIdx.x;
    const int per_tile = a.row_regions * a.col_regions;
    const int64_t tile = blockIdx.x / (unsigned)per_tile;
    const int within = (int)(blockIdx.x % (unsigned)per_tile);
    jb::JpegRegion g;
    g.height = (int)a.height;
    g.width = (int)a.width;
    g.sub = a.sub;
    g.y0 = (within / a.col_regions) * g.region_h();
    g.x0 = (within % a.col_regions) * jb::kJpegRegionW;
    const int64_t width = a.width, pixels = a.height * a.width;
    const T* img = images + tile * 3 * pixels;
    O* dst = out + tile * 3 * pixels;
    const int rows_in = g.rows_in(), cols_in = g.cols_in();
    auto element = [&](int c, int64_t p) -> int64_t {      // channel c of pixel p of the tile
        if constexpr (kInter) return p * 3 + c; else return c * pixels + p;
    };

    // ---- 0. the quality
    const int quality = jb::jpeg_quality(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.qualities[a.per_row ? tile : 0]))));
    if (quality == 0) {      // ---- a copy tile: the region's elements streamed through (uniform in the workgroup: nobody waits at a barrier below)
        const int lines = kInter ? rows_in : 3 * rows_in, length = kInter ? 3 * cols_in : cols_in;      // NHWC: a row of the region is 3 * cols_in consecutive elements
        auto line_start = [&](int line) -> int64_t {
            if constexpr (kInter) return ((g.y0 + line) * width + g.x0) * 3; else return (int64_t)(line / rows_in) * pixels + (g.y0 + line % rows_in) * width + g.x0;
        };
        if (a.vec_copy) {      // (width % 4 == 0: every line starts on a pack and is a whole number of packs)
            const int packs = length / 4;
            for (int i = tid; i < lines * packs; i += kJpegThreads) {
                const int64_t at = line_start(i / packs) + 4 * (i % packs);
                const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(img + at);
                O res[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) res[e] = jpeg_copy<T, O, kUnit>(pk.v[e]);
                store_pack_stream<O, 4>(dst + at, res);
            }
        } else {
            for (int i = tid; i < lines * length; i += kJpegThreads) {
                const int64_t at = line_start(i / length) + i % length;
                dst[at] = jpeg_copy<T, O, kUnit>(img[at]);
            }
        }
        return;
    }
    if (tid < 128) {
        const int entry = jb::jpeg_table_entry(quality, tid >> 6, tid & 63);
        table_q[tid] = (uint16_t)entry;
        table_m[tid] = jb::jpeg_magic(entry);
    }

    // Four neighbouring pixels of source row `row`, the first at column x (inside the tile where `pack`): their levels.
    auto load_quad = [&](int row, int x, bool pack, auto&& column, int (&lv)[3][4]) {
        const int64_t line = (int64_t)row * width;
        if (pack) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(img + c * pixels + line + x);
#pragma unroll
                for (int e = 0; e < 4; ++e) lv[c][e] = jpeg_level_of<T>(pk.v[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t p = line + column(e);
#pragma unroll
                for (int c = 0; c < 3; ++c) lv[c][e] = jpeg_level_of<T>(img[element(c, p)]);
            }
        }
    };

    // ---- 1. colour: the full-resolution planes of the region, whole blocks
    {
        const int rows_coded = g.rows_coded(), quads = g.cols_coded() / 4;
        for (int i = tid; i < rows_coded * quads; i += kJpegThreads) {
            const int lr = i / quads, lx = 4 * (i % quads);
            int lv[3][4];
            load_quad(g.source_row(lr), g.x0 + lx, a.vec_in && g.x0 + lx + 3 < g.width, [&](int e) { return g.source_col(lx + e); }, lv);
            uint32_t wy = 0u, wb = 0u, wr = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                wy |= (uint32_t)jb::jpeg_luma(lv[0][e], lv[1][e], lv[2][e]) << (8 * e);
                if (g.sub == 0) {
                    wb |= (uint32_t)jb::jpeg_cb(lv[0][e], lv[1][e], lv[2][e]) << (8 * e);
                    wr |= (uint32_t)jb::jpeg_cr(lv[0][e], lv[1][e], lv[2][e]) << (8 * e);
                }
            }
            uint8_t* at = planes + lr * jb::kJpegPitch + lx;
            *reinterpret_cast<uint32_t*>(at) = wy;
            if (g.sub == 0) {
                *reinterpret_cast<uint32_t*>(at + jb::kJpegPlaneBytes444) = wb;
                *reinterpret_cast<uint32_t*>(at + 2 * jb::kJpegPlaneBytes444) = wr;
            }
        }
    }
    if (g.sub != 0) {      // 4:2:0: the chroma window, two samples (2 x 4 pixels) per thread
        const int lo_y = g.win_lo_y(), lo_x = g.win_lo_x(), rows = g.win_hi_y() - lo_y, pairs = (g.win_hi_x() - lo_x) / 2;
        for (int i = tid; i < rows * pairs; i += kJpegThreads) {
            const int ly = lo_y + i / pairs, lx = lo_x + 2 * (i % pairs);
            const int cx = g.win_x() + lx, x = 2 * cx;
            int source[2];
            g.chroma_rows(g.win_y() + ly, source);
            const int upper = source[0], lower = source[1];
            int b_left = 0, b_right = 0, r_left = 0, r_right = 0;      // the sums of the two samples (scalars: an array indexed in a loop went to scratch)
            auto add_row = [&](int row) {
                int lv[3][4];
                load_quad(row, x, a.vec_in && x + 3 < g.width, [&](int e) { return g.chroma_col(x + e); }, lv);
                b_left += jb::jpeg_cb(lv[0][0], lv[1][0], lv[2][0]) + jb::jpeg_cb(lv[0][1], lv[1][1], lv[2][1]);
                b_right += jb::jpeg_cb(lv[0][2], lv[1][2], lv[2][2]) + jb::jpeg_cb(lv[0][3], lv[1][3], lv[2][3]);
                r_left += jb::jpeg_cr(lv[0][0], lv[1][0], lv[2][0]) + jb::jpeg_cr(lv[0][1], lv[1][1], lv[2][1]);
                r_right += jb::jpeg_cr(lv[0][2], lv[1][2], lv[2][2]) + jb::jpeg_cr(lv[0][3], lv[1][3], lv[2][3]);
            };
            add_row(upper);
            add_row(lower);
            // (jpeg_chroma_mean's bias: 1 in the even column cx, 2 in the odd column cx + 1 -- the window starts on an even sample)
            uint8_t* at = planes + jb::kJpegLumaBytes420 + ly * jb::kJpegChromaPitch + lx;
            *reinterpret_cast<uint16_t*>(at) = (uint16_t)(jb::jpeg_chroma_mean(b_left, 0, 0, 0, cx) | (jb::jpeg_chroma_mean(b_right, 0, 0, 0, cx + 1) << 8));
            *reinterpret_cast<uint16_t*>(at + jb::kJpegChromaBytes420) = (uint16_t)(jb::jpeg_chroma_mean(r_left, 0, 0, 0, cx) | (jb::jpeg_chroma_mean(r_right, 0, 0, 0, cx + 1) << 8));
        }
    }
    __syncthreads();

    // ---- 2. blocks: one thread codes one block, in place
    for (int j = tid; j < g.jobs(); j += kJpegThreads) {
        int offset, pitch, chroma;
        if (!g.job(j, offset, pitch, chroma)) continue;
        uint8_t* block = planes + offset;
        int v[64];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint2 w = *reinterpret_cast<const uint2*>(block + r * pitch);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[8 * r + e] = (int)((w.x >> (8 * e)) & 0xFFu);
                v[8 * r + 4 + e] = (int)((w.y >> (8 * e)) & 0xFFu);
            }
        }
        jb::jpeg_code_block(v, table_q + 64 * chroma, table_m + 64 * chroma);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 w = make_uint2(0u, 0u);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w.x |= (uint32_t)v[8 * r + e] << (8 * e);
                w.y |= (uint32_t)v[8 * r + 4 + e] << (8 * e);
            }
            *reinterpret_cast<uint2*>(block + r * pitch) = w;
        }
    }
    __syncthreads();

    // ---- 3. output: four neighbouring pixels of a row per thread
    const uint8_t* msk = tile_mask(mk, tile, pixels);
    const bool replicate = g.chroma_w() <= 2;
    const int quads = (cols_in + 3) / 4;
    for (int i = tid; i < rows_in * quads; i += kJpegThreads) {
        const int lr = i / quads, lx = 4 * (i % quads);
        const uint32_t wy = *reinterpret_cast<const uint32_t*>(planes + lr * jb::kJpegPitch + lx);
        int cb[4], cr[4];
        if (g.sub == 0) {
            const uint32_t wb = *reinterpret_cast<const uint32_t*>(planes + jb::kJpegPlaneBytes444 + lr * jb::kJpegPitch + lx);
            const uint32_t wr = *reinterpret_cast<const uint32_t*>(planes + 2 * jb::kJpegPlaneBytes444 + lr * jb::kJpegPitch + lx);
#pragma unroll
            for (int e = 0; e < 4; ++e) cb[e] = (int)((wb >> (8 * e)) & 0xFFu), cr[e] = (int)((wr >> (8 * e)) & 0xFFu);
        } else {
            const int y = g.y0 + lr, cx = (g.x0 + lx) >> 1;
            const uint8_t* row_near = planes + jb::kJpegLumaBytes420 + (g.up_row(y) - g.win_y()) * jb::kJpegChromaPitch;
            const uint8_t* row_other = planes + jb::kJpegLumaBytes420 + (g.up_other_row(y) - g.win_y()) * jb::kJpegChromaPitch;
            int near_b[4], other_b[4], near_r[4], other_r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col = g.up_col(cx, k) - g.win_x();      // (window-local)
                near_b[k] = row_near[col], other_b[k] = row_other[col];
                near_r[k] = row_near[jb::kJpegChromaBytes420 + col], other_r[k] = row_other[jb::kJpegChromaBytes420 + col];
            }
            jb::jpeg_chroma_up4(near_b, other_b, replicate, cb);
            jb::jpeg_chroma_up4(near_r, other_r, replicate, cr);
        }
        O res[3][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int rgb[3];
            jb::jpeg_to_rgb((int)((wy >> (8 * e)) & 0xFFu), cb[e], cr[e], rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c][e] = hsv_to_output<T, O, kUnit>((float)rgb[c]);
        }
        const int gx = g.x0 + lx;
        const int64_t p = (int64_t)(g.y0 + lr) * width + gx;      // the first of the four pixels
        if constexpr (kMask) {      // a masked-out pixel: the input element, copied
            uint32_t bytes = 0u;
            if (a.mask_vec) {
                bytes = *reinterpret_cast<const uint32_t*>(msk + p);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (gx + e < g.width) bytes |= (msk[p + e] != 0 ? 1u : 0u) << (8 * e);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (gx + e < g.width && ((bytes >> (8 * e)) & 0xFFu) == 0u) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) res[c][e] = jpeg_copy<T, O, kUnit>(img[c * pixels + p + e]);
                }
        }
        if (a.vec_out) {      // (width % 4 == 0: the quad lies inside the row)
#pragma unroll
            for (int c = 0; c < 3; ++c) store_pack_stream<O, 4>(dst + c * pixels + p, res[c]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (gx + e < g.width) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[element(c, p + e)] = res[c][e];
                }
        }
    }
}

template <typename T, bool kMask = false>
static int jpeg_roundtrip_typed(const void* images, void* out, JpegArgs a, int out_code, bool interleaved, bool unit, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    const bool quads = a.width % 4 == 0;
    const bool in_ok = quads && aligned_for(images, 4 * sizeof(T)), out_ok = quads && aligned_for(out, 4 * out_elem_bytes(sizeof(T), out_code, unit));
    a.vec_in = in_ok && !interleaved;
    a.vec_out = out_ok && !interleaved;
    a.vec_copy = in_ok && out_ok;
    if constexpr (kMask) a.mask_vec = quads && aligned_for(mk.mask, 4);
    const T* in = static_cast<const T*>(images);
    const unsigned grid = (unsigned)(a.n_tiles * a.row_regions * a.col_regions);
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<1, kMask>(false, interleaved, [&](auto, auto inter) {
            hipLaunchKernelGGL((jpeg_roundtrip_kernel<T, O, decltype(u)::value, decltype(inter)::value, kMask>), dim3(grid), dim3(kJpegThreads), 0, stream, in, static_cast<O*>(out), a, mk);
            return check_launch("jpeg round trip");
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
template <bool kMask>
static int jpeg_roundtrip_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* qualities, int64_t n_rows, int subsampling,
                               const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    const char* who = kMask ? "sx_jpeg_roundtrip_masked" : "sx_jpeg_roundtrip";
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    int rc = check_tiles(n, h, w);
    if (rc != SX_OK) return rc;
    if (!qualities) return fail(SX_ERR_BAD_ARG, "qualities pointer is null");
    if ((rc = check_rows("n_rows", n_rows, n)) != SX_OK) return rc;
    if (subsampling != 0 && subsampling != 2) return fail(SX_ERR_BAD_ARG, "subsampling must be 0 (4:4:4) or 2 (4:2:0), got %d", subsampling);
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    rc = deconv_flags_ok(flags, dtype, kMask, who);
    if (rc != SX_OK) return rc;
    JpegArgs a{};
    a.qualities = qualities;
    a.height = h;
    a.width = w;
    a.n_tiles = n;
    a.per_row = rows_per_tile(n_rows, n);
    a.sub = subsampling;
    const int64_t region_h = subsampling ? sx::jpeg_block::kJpegRegionH420 : sx::jpeg_block::kJpegRegionH444;
    const int64_t row_regions = (h + region_h - 1) / region_h, col_regions = (w + sx::jpeg_block::kJpegRegionW - 1) / sx::jpeg_block::kJpegRegionW;
    if (n * row_regions * col_regions > 0x7fffffffll || h > 0x7fffff00ll || w > 0x7fffff00ll) return fail(SX_ERR_BAD_ARG, "images too large for one call");      // (coordinates are ints)
    a.row_regions = (int)row_regions;
    a.col_regions = (int)col_regions;
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return jpeg_roundtrip_typed<typename decltype(t)::type, kMask>(images, out, a, out_code, inter, unit, stream, mk); });
}

extern "C" int sx_jpeg_roundtrip(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* qualities, int64_t n_rows, int subsampling, unsigned flags,
                                 void* stream_ptr) {
    return jpeg_roundtrip_call<false>(images, out, dtype, n, h, w, qualities, n_rows, subsampling, nullptr, flags, stream_ptr);
}

extern "C" int sx_jpeg_roundtrip_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* qualities, int64_t n_rows, int subsampling,
                                        const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    return jpeg_roundtrip_call<true>(images, out, dtype, n, h, w, qualities, n_rows, subsampling, mask_dev, flags, stream_ptr);
}
