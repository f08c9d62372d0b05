// Gaussian blur with a sigma per tile (sx_gaussian_blur / sx_gaussian_blur_masked) -- included at the end of macenko.hip next to hsv.hpp,
// whose helpers it uses as they are: raw_value, rgb_to_output, MaskArgs / tile_mask, store_pack_stream, with_out / with_layout.  DESIGN.md 4s.
//
// THE RULE.  Per tile ONE float32 sigma is read from device memory.  Each channel plane is filtered on its own and a pixel never sees
// another tile.
//   Radius   R = min((int)(4 sigma + 0.5), 16) of the float32 sigma: scipy.ndimage.gaussian_filter's rule with truncate = 4.0.  The sum is
//            taken EXACTLY (in float64, which holds 4 sigma + 0.5 of every float32 sigma up to 4): rounded to float32 the sum of the float
//            just below 0.125 is a tie that goes up to 1.0, and "sigma < 0.125 copies" would be off by one float.
//            kBlurMaxSigma = 4.0f: a larger FINITE sigma is clamped to 4 (R = 16) -- the rows live on the device and cannot be refused
//            without a synchronisation.
//   Taps     w_i = exp(-i^2 / (2 sigma^2)) for i = -R..R, divided by their sum, in float32.  All taps are positive: the filter is a convex
//            combination, nothing is clamped and a constant tile stays constant.
//   Borders  reflected WITHOUT repeating the edge, inside the pixel's own tile, folded as often as needed: period 2 (n - 1), an axis of
//            length 1 maps to 0 -- focus.hpp's rule for radii larger than the axis; scipy's mode="mirror", torch's "reflect" padding.
//   Arithmetic  separable, rows then columns, float32, on the values as the element type stores them: a uint8 byte is its level 0..255, a
//            float element is taken AS IT IS (no x 255: the filter is linear, the scale is the caller's).  Each pass evaluates
//            acc = w_0 x_0;  acc = fma(w_i, x_-i + x_+i, acc) for i = 1..R  (the taps are symmetric: R + 1 products, not 2 R + 1).
//   Output   through the output rule of the sibling calls (rgb_to_output: the cast, SX_MACENKO_OUT_BF16 / _OUT_F16, the / 255 of
//            SX_MACENKO_NORMALIZE_0_1).  An 8-bit level is ROUNDED TO NEAREST as in hsv.hpp, not truncated.
//   Copies   a tile whose sigma is NaN, infinite or <= 0, a tile whose R is 0 (sigma < 0.125) and -- masked call -- a masked-out pixel
//            are copied: the stored element through the output rule, with NO clamp.  Where the output element is the input element and
//            nothing is divided, that is the element's bits (float tiles: NaN payloads and -0.0 included).
//   Non-finite pixels are not special: they go through the window as IEEE arithmetic takes them, as in scipy -- a NaN pixel spreads over
//            its (2 R + 1)^2 window, and over nothing else.
//   Masks    planar tiles only.  The mask selects which OUTPUT pixels are written from the blur; the taps read every pixel and the
//            weights are not renormalised.
//
// THE KERNEL.  ONE launch per call: no workspace, no atomics, no memset.  A workgroup of 256 threads takes a 64 x 64 output block of one
// tile, reads the tile's sigma (every lane the same word, then readfirstlane: R and the 17 taps are wave-uniform scalars) and, for a copy
// tile, streams its block through.  Otherwise, channel after channel:
//   1. stage   the block with an R-pixel halo -- (rows + 2 R) x (64 + 2 R) values, the tile's own R, not 16 -- as float32 in `stage_a`,
//              every coordinate reflected as it is staged (two tables of folded coordinates, made once per workgroup): no load leaves the
//              tile and the border rule costs nothing later.  Aligned planar input loads 4-pixel packs; the halo columns, unaligned views
//              and NHWC take single elements.  The block's first column always sits at float 16 of a staged row, so packs are 16-byte
//              stores and the row pass reads aligned quads whatever R is.
//   2. rows    a thread takes four neighbouring outputs of a staged row: it reads the (4 + 2 R) values they need as aligned 16-byte
//              quads into registers (at most nine), and writes the four sums as one quad to `stage_b`, (rows + 2 R) x 64.
//   3. columns a thread takes four neighbouring columns of an output row: 2 R + 1 quads of `stage_b`, one per tap, and writes the
//              output pack (or single elements).
// LDS: stage_a 96 x 96 and stage_b 96 x 64 floats = 60 KB, the two tables 1.5 KB: 61.5 KB, two workgroups per CU (160 KB).
// Banks (ds_read_b128 / ds_write_b128: groups of 16 lanes, bank = dword mod 64; a group takes lanes 0-3 and 12-15 of one sixteen and 4-11
// of the next): sixteen lanes read the 64 consecutive dwords of one row, so a group is conflict-free when its two rows start a multiple of
// 64 dwords apart.  stage_b's pitch is 64: any two rows do.  stage_a's pitch is 96 (a pitch of 128 would not fit 64 KB): the two sixteens
// of a half-wave take rows TWO apart (192 dwords) -- blur_row_of() -- in both passes.
namespace sx {
namespace macenko {

constexpr float kBlurMaxSigma = 4.0f;
constexpr int kBlurMaxRadius = 16;
constexpr int kBlurSide = 64;                                        // the output block
constexpr int kBlurThreads = 256;
constexpr int kBlurStaged = kBlurSide + 2 * kBlurMaxRadius;          // 96: rows and columns of the staged block at R = 16
constexpr int kBlurPitchA = kBlurStaged;                             // floats of a staged row
constexpr int kBlurPitchB = kBlurSide;                               // floats of a row of the row pass's result
constexpr int kBlurFirst = kBlurMaxRadius;                           // the float of a staged row that holds the block's first column
constexpr int kBlurQuads = kBlurSide / 4;                            // threads per row in the two passes
static_assert(kBlurFirst % 4 == 0 && kBlurPitchA % 4 == 0 && kBlurPitchB % 64 == 0 && (2 * kBlurPitchA) % 64 == 0, "aligned quads; rows of a group a multiple of 64 dwords apart");
static_assert((kBlurStaged * (kBlurPitchA + kBlurPitchB)) * sizeof(float) + 2 * kBlurStaged * sizeof(int64_t) <= 63 * 1024, "a workgroup stays within 64 KB of LDS");

struct BlurArgs {
    const float* sigmas;          // n_rows floats
    int64_t height, width, n_tiles;
    int row_blocks, col_blocks;   // workgroups per tile
    int per_row;                  // 1: sigma `tile`, 0: one sigma for the batch
    int vec_in, vec_out;          // planar: 4-pixel packs of the input / of the output
    int vec_copy;                 // the copy path's packs (either layout)
    int mask_vec;                 // the mask's four bytes as one word
};

__host__ __device__ inline int blur_radius(float sigma) {      // sigma finite, > 0, <= kBlurMaxSigma
    const int r = (int)(4.0 * (double)sigma + 0.5);      // (exact: see the rule)
    return r < kBlurMaxRadius ? r : kBlurMaxRadius;
}

// rgb_to_output with the 8-bit level rounded to nearest (hsv.hpp's rule).
template <typename T, typename O, bool kUnit>
__device__ __forceinline__ O blur_to_output(float level) {
    if constexpr (sizeof(T) == 1) level = rintf(level);
    return rgb_to_output<T, O, kUnit>(level);
}

// A copied element: its bits where nothing converts it, the output rule on its value otherwise.
template <typename T, typename O, bool kUnit>
__device__ __forceinline__ O blur_copy(T v) {
    if constexpr (std::is_same<T, O>::value && !kUnit) return v; else return rgb_to_output<T, O, kUnit>(raw_value<T>(v));
}

// The row of the q-th group of four rows that the lanes of sixteen `sub` (0..3 within the wave) take: 0, 2, 1, 3.
__device__ __forceinline__ int blur_row_of(int q, int sub) { return 4 * q + (((sub & 1) << 1) | (sub >> 1)); }

// acc = w_0 x_0 + sum_i w_i (x_-i + x_+i) for four neighbouring outputs; at(k) is the quad of values at distance k.
#define SX_BLUR_TAPS(R, w, acc, centre, minus, plus)                                                  \
    _Pragma("unroll") for (int o = 0; o < 4; ++o) acc[o] = w[0] * (centre);                           \
    _Pragma("unroll") for (int i = 1; i <= kBlurMaxRadius; ++i) {                                     \
        if (i <= R) {      /* (uniform; no early exit: the loop unrolls and every index is a constant) */ \
            _Pragma("unroll") for (int o = 0; o < 4; ++o) acc[o] = fmaf(w[i], (minus) + (plus), acc[o]);  \
        }                                                                                             \
    }

template <typename T, typename O, bool kUnit, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kBlurThreads) void gaussian_blur_kernel(const T* __restrict__ images, O* __restrict__ out, BlurArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
#pragma clang fp contract(off)      // (every fused multiply-add is written out)
    static_assert(!(kInter && kMask), "the masked forms are planar");
    __shared__ __attribute__((aligned(16))) float stage_a[kBlurStaged * kBlurPitchA];
    __shared__ __attribute__((aligned(16))) float stage_b[kBlurStaged * kBlurPitchB];
    __shared__ int64_t fold_y[kBlurStaged], fold_x[kBlurStaged];
    const int tid = threadIdx.x;
    const int per_tile = a.row_blocks * a.col_blocks;
    const int64_t tile = blockIdx.x / (unsigned)per_tile;
    const int within = (int)(blockIdx.x % (unsigned)per_tile);
    const int64_t y0 = (int64_t)(within / a.col_blocks) * kBlurSide, x0 = (int64_t)(within % a.col_blocks) * kBlurSide;
    const int64_t height = a.height, width = a.width, pixels = height * width;
    const T* img = images + tile * 3 * pixels;
    O* dst = out + tile * 3 * pixels;
    const int rows_in = (int)min((int64_t)kBlurSide, height - y0), cols_in = (int)min((int64_t)kBlurSide, width - x0);      // the block inside the tile

    auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    float sigma = uniform(a.sigmas[a.per_row ? tile : 0]);
    const bool finite_positive = sigma > 0.0f && sigma < __builtin_huge_valf();      // (false for a NaN)
    sigma = fminf(sigma, kBlurMaxSigma);
    const int R = finite_positive ? blur_radius(sigma) : 0;

    if (R == 0) {      // ---- a copy tile: the block's elements streamed through (uniform in the workgroup: nobody waits at a barrier below)
        const int lines = kInter ? rows_in : 3 * rows_in, length = kInter ? 3 * cols_in : cols_in;      // NHWC: a row of the block is 3 * cols_in consecutive elements
        auto line_start = [&](int line) -> int64_t {
            if constexpr (kInter) return ((y0 + line) * width + x0) * 3; else return (int64_t)(line / rows_in) * pixels + (y0 + line % rows_in) * width + x0;
        };
        if (a.vec_copy) {      // (width % 4 == 0: every line starts on a pack and is a whole number of packs)
            const int packs = length / 4;
            for (int i = tid; i < lines * packs; i += kBlurThreads) {
                const int64_t at = line_start(i / packs) + 4 * (i % packs);
                const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(img + at);
                O res[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) res[e] = blur_copy<T, O, kUnit>(pk.v[e]);
                store_pack_stream<O, 4>(dst + at, res);
            }
        } else {
            for (int i = tid; i < lines * length; i += kBlurThreads) {
                const int64_t at = line_start(i / length) + i % length;
                dst[at] = blur_copy<T, O, kUnit>(img[at]);
            }
        }
        return;
    }

    // ---- the taps: every lane computes the same seventeen, they are held as scalars
    float w[kBlurMaxRadius + 1];
    {
        const float scale = -0.5f / (sigma * sigma);
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i <= kBlurMaxRadius; ++i) {
            w[i] = i <= R ? expf((float)(i * i) * scale) : 0.0f;
            sum += i == 0 ? w[i] : 2.0f * w[i];
        }
#pragma unroll
        for (int i = 0; i <= kBlurMaxRadius; ++i) w[i] = uniform(w[i] / sum);
    }

    // ---- the folded coordinates of the staged rows and columns
    const int side = kBlurSide + 2 * R, rows_staged = rows_in + 2 * R;
    if (tid < 2 * kBlurStaged) {
        const bool is_x = tid >= kBlurStaged;
        const int k = is_x ? tid - kBlurStaged : tid;
        const int64_t n = is_x ? width : height;
        int64_t q = 0;
        if (n > 1 && k < side) {
            const int64_t period = 2 * (n - 1);
            q = ((is_x ? x0 : y0) - R + k) % period;
            q = q < 0 ? q + period : q;
            q = q >= n ? period - q : q;
        }
        (is_x ? fold_x : fold_y)[k] = q;
    }
    __syncthreads();

    const int64_t step = kInter ? 3 : 1;
    const int sub = (tid >> 4) & 3, quad = tid & (kBlurQuads - 1);      // the sixteen within the wave, the quad of columns
    const int first_chunk = (kBlurFirst - R) >> 2, last_chunk = (kBlurFirst + 3 + R) >> 2;      // the quads of a row-pass window that hold a needed value
    const uint8_t* msk = tile_mask(mk, tile, pixels);

    for (int c = 0; c < 3; ++c) {
        const T* plane = img + (kInter ? (int64_t)c : c * pixels);
        // ---- 1. stage (the barrier after the previous channel's row pass has passed: nobody reads stage_a any more)
        if (a.vec_in) {
            for (int i = tid; i < rows_staged * kBlurQuads; i += kBlurThreads) {
                const int sr = i / kBlurQuads, j = i % kBlurQuads;
                const int64_t line = fold_y[sr] * width;
                float v[4];
                if (x0 + 4 * j < width) {      // (width % 4 == 0: the pack lies inside the row)
                    load_raw<T, 4>(plane + line + x0 + 4 * j, v);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = raw_value<T>(plane[line + fold_x[R + 4 * j + e]]);
                }
                *reinterpret_cast<float4*>(&stage_a[sr * kBlurPitchA + kBlurFirst + 4 * j]) = make_float4(v[0], v[1], v[2], v[3]);
            }
            for (int i = tid; i < rows_staged * 2 * R; i += kBlurThreads) {      // the halo columns
                const int sr = i / (2 * R), k = i % (2 * R), sc = k < R ? k : kBlurSide + k;
                stage_a[sr * kBlurPitchA + kBlurFirst - R + sc] = raw_value<T>(plane[fold_y[sr] * width + fold_x[sc]]);
            }
        } else {
            for (int i = tid; i < rows_staged * side; i += kBlurThreads) {
                const int sr = i / side, sc = i % side;
                stage_a[sr * kBlurPitchA + kBlurFirst - R + sc] = raw_value<T>(plane[(fold_y[sr] * width + fold_x[sc]) * step]);
            }
        }
        __syncthreads();

        // ---- 2. rows: stage_a -> stage_b (the barrier after the previous channel's staging has passed: nobody reads stage_b any more)
        for (int q = tid >> 6; 4 * q < rows_staged; q += kBlurThreads / kWave) {
            const int sr = blur_row_of(q, sub);
            if (sr < rows_staged) {
                float win[4 * (2 * kBlurMaxRadius / 4 + 1)];      // win[k]: the staged float 4 * quad + k; output o is win[kBlurFirst + o]
#pragma unroll
                for (int m = 0; m < 2 * kBlurMaxRadius / 4 + 1; ++m) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (m >= first_chunk && m <= last_chunk) v = *reinterpret_cast<const float4*>(&stage_a[sr * kBlurPitchA + 4 * quad + 4 * m]);
                    win[4 * m] = v.x, win[4 * m + 1] = v.y, win[4 * m + 2] = v.z, win[4 * m + 3] = v.w;
                }
                float acc[4];
                SX_BLUR_TAPS(R, w, acc, win[kBlurFirst + o], win[kBlurFirst + o - i], win[kBlurFirst + o + i])
                *reinterpret_cast<float4*>(&stage_b[sr * kBlurPitchB + 4 * quad]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        }
        __syncthreads();

        // ---- 3. columns: stage_b -> the output
        for (int q = tid >> 6; 4 * q < rows_in; q += kBlurThreads / kWave) {
            const int r = blur_row_of(q, sub);
            const int64_t gx = x0 + 4 * quad;
            if (r < rows_in && gx < width) {
                const float* column = &stage_b[(r + R) * kBlurPitchB + 4 * quad];
                float taps[2 * kBlurMaxRadius + 1][4];      // taps[kBlurMaxRadius + k]: the quad k rows away; all of them requested before the first is used
                auto fetch = [&](int k) {
                    const float4 v = *reinterpret_cast<const float4*>(column + k * kBlurPitchB);
                    float* t = taps[kBlurMaxRadius + k];
                    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
                };
                fetch(0);
#pragma unroll
                for (int i = 1; i <= kBlurMaxRadius; ++i) {
                    if (i <= R) {
                        fetch(-i);
                        fetch(i);
                    }
                }
                float acc[4];
                SX_BLUR_TAPS(R, w, acc, taps[kBlurMaxRadius][o], taps[kBlurMaxRadius - i][o], taps[kBlurMaxRadius + i][o])
                const int64_t p = (y0 + r) * width + gx;      // the first of the four pixels
                O res[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) res[o] = blur_to_output<T, O, kUnit>(acc[o]);
                if constexpr (kMask) {      // a masked-out pixel: the input element, copied
                    uint32_t bytes = 0u;
                    if (a.mask_vec) {
                        bytes = *reinterpret_cast<const uint32_t*>(msk + p);
                    } else {
#pragma unroll
                        for (int o = 0; o < 4; ++o)
                            if (gx + o < width) bytes |= (msk[p + o] != 0 ? 1u : 0u) << (8 * o);
                    }
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        if (gx + o < width && ((bytes >> (8 * o)) & 0xFFu) == 0u) res[o] = blur_copy<T, O, kUnit>(plane[p + o]);
                }
                if (a.vec_out) {
                    store_pack_stream<O, 4>(dst + c * pixels + p, res);
                } else {
                    O* to = dst + (kInter ? (int64_t)c : c * pixels);
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        if (gx + o < width) to[(p + o) * step] = res[o];
                }
            }
        }
    }
}
#undef SX_BLUR_TAPS

template <typename T, bool kMask = false>
static int gaussian_blur_typed(const void* images, void* out, BlurArgs a, int out_code, bool interleaved, bool unit, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    const bool quads = a.width % 4 == 0;
    const bool in_ok = quads && aligned_for(images, 4 * sizeof(T)), out_ok = quads && aligned_for(out, 4 * out_elem_bytes(sizeof(T), out_code, unit));
    a.vec_in = in_ok && !interleaved;
    a.vec_out = out_ok && !interleaved;
    a.vec_copy = in_ok && out_ok;
    if constexpr (kMask) a.mask_vec = quads && aligned_for(mk.mask, 4);
    const T* in = static_cast<const T*>(images);
    const unsigned grid = (unsigned)(a.n_tiles * a.row_blocks * a.col_blocks);
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<1, kMask>(false, interleaved, [&](auto, auto inter) {
            hipLaunchKernelGGL((gaussian_blur_kernel<T, O, decltype(u)::value, decltype(inter)::value, kMask>), dim3(grid), dim3(kBlurThreads), 0, stream, in, static_cast<O*>(out), a, mk);
            return check_launch("gaussian blur");
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
template <bool kMask>
static int gaussian_blur_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* sigmas, int64_t n_rows, const unsigned char* mask_dev, unsigned flags,
                              void* stream_ptr) {
    const char* who = kMask ? "sx_gaussian_blur_masked" : "sx_gaussian_blur";
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    int rc = check_tiles(n, h, w);
    if (rc != SX_OK) return rc;
    if (!sigmas) return fail(SX_ERR_BAD_ARG, "sigmas pointer is null");
    if ((rc = check_rows("n_rows", n_rows, n)) != SX_OK) return rc;
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    rc = deconv_flags_ok(flags, dtype, kMask, who);
    if (rc != SX_OK) return rc;
    BlurArgs a{};
    a.sigmas = sigmas;
    a.height = h;
    a.width = w;
    a.n_tiles = n;
    a.per_row = rows_per_tile(n_rows, n);
    const int64_t row_blocks = (h + kBlurSide - 1) / kBlurSide, col_blocks = (w + kBlurSide - 1) / kBlurSide;
    if (n * row_blocks * col_blocks > 0x7fffffffll) return fail(SX_ERR_BAD_ARG, "images too large for one call");      // (n * h * w < 2^32: each factor fits an int)
    a.row_blocks = (int)row_blocks;
    a.col_blocks = (int)col_blocks;
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return gaussian_blur_typed<typename decltype(t)::type, kMask>(images, out, a, out_code, inter, unit, stream, mk); });
}

extern "C" int sx_gaussian_blur(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* sigmas, int64_t n_rows, unsigned flags, void* stream_ptr) {
    return gaussian_blur_call<false>(images, out, dtype, n, h, w, sigmas, n_rows, nullptr, flags, stream_ptr);
}

extern "C" int sx_gaussian_blur_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* sigmas, int64_t n_rows, const unsigned char* mask_dev,
                                       unsigned flags, void* stream_ptr) {
    return gaussian_blur_call<true>(images, out, dtype, n, h, w, sigmas, n_rows, mask_dev, flags, stream_ptr);
}
