// HSV colour jitter: per-tile hue, saturation and value (sx_hsv_apply / sx_hsv_apply_masked) -- included at the end of macenko.hip next to
// deconv.hpp, whose streaming helpers it uses as they are: deconv_load / load_pixels, store_pixels, store_pixels_staged, MaskArgs /
// MaskPack / tile_mask, input_level, rgb_to_output, kStreamThreads.  DESIGN.md 4r.
//
// A row is 5 floats (dh, a_s, b_s, a_v, b_v), dh in turns.  All arithmetic is float32 on 0-255 levels; r, g, b are the input levels
// (input_level<T>) clamped to [0, 255]:
//   M = max, m = min, C = M - m;   s = C / M (0 where M <= 0)
//   h6 in [0, 6): 0 where C == 0; (g - b) / C (+ 6 if negative) where M == r; 2 + (b - r) / C where M == g; 4 + (r - g) / C otherwise
//   h6' = h6 + 6 dh reduced into [0, 6) by x - 6 floor(x / 6);   s' = clamp(a_s s + b_s, 0, 1);   V' = 255 clamp(a_v M / 255 + b_v, 0, 1)
//   n = 5, 3, 1 for r, g, b:  k = h6' + n (- 6 where k >= 6),  t = clamp(min(k, 4 - k), 0, 1),  out = V' - V' s' t
// The kernel evaluates three parts in an algebraically equal, shorter form (the rule above is what tests/_hsv_numpy.py restates in float64):
// V' = clamp(a_v M + 255 b_v, 0, 255), no quotient by 255; the "+ 6 if negative" of h6 is left to the reduction of h6'; and t without the
// wrap of k: 2 - |h6' - 3| for r, |h6' - 2| - 1 for g, |h6' - 4| - 1 for b, clamped to [0, 1].  The two quotients: hsv_quotient below.
//
// The output rule.  A float element gets the level through rgb_to_output's float branches (the / 255 fusion included).  An 8-bit level --
// uint8 output, and the uint8 level rgb_to_output quantises a uint8 tile's result to before it casts it to bf16 / f16 or divides it by 255 --
// is ROUNDED TO NEAREST (rintf), not truncated as the stain kernels truncate theirs: the float32 round trip RGB -> HSV -> RGB of the identity
// row (0, 1, 0, 1, 0) is off by up to 1.8e-4 of a level, so truncation would turn some of the 2^24 uint8 colours one level down, while
// rounding returns every one of them exactly.  The stain kernels keep their truncation.
//
// Copies.  A pixel with a NaN in any channel, a masked-out pixel and every pixel of a tile whose row has a non-finite member are copied by
// the background rule of the masked transforms: the input level through the clamp, the cast and / 255 (uint8 in, uint8 out: the same bytes).
// Every use of a value that may be NaN is a select, never a product with zero.
//
// ONE launch per call: no workspace, no atomics, no memset, no LDS beyond the row (and the staging area of the interleaved stores).
namespace sx {
namespace macenko {

struct HsvArgs {
    const float* rows;        // n_rows x 5: (dh, a_s, b_s, a_v, b_v)
    int64_t pixels, n_tiles;  // P = H*W, N
    int chunk, blocks;        // pixels per work item, work items per tile
    int per_row;              // 1: row `tile`, 0: one row for the batch
};

// rgb_to_output with the 8-bit level rounded to nearest where the rule quantises to one (see the header comment).
template <typename T, typename O, bool kUnit>
__device__ __forceinline__ O hsv_to_output(float level) {
    if constexpr (sizeof(T) == 1) level = rintf(level);
    return rgb_to_output<T, O, kUnit>(level);
}

// num / den for den > 0.  Levels of a uint8 tile are integers, C and M at least 1: the hardware's reciprocal (v_rcp_f32, one unit in the last
// place) and a product.  A float tile may hold levels down to the denormals, where that reciprocal overflows: the IEEE quotient there.
template <typename T>
__device__ __forceinline__ float hsv_quotient(float num, float den) {
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 1) return num * __builtin_amdgcn_rcpf(den); else return num / den;
}

template <typename T, typename O, int V, bool kUnit, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kStreamThreads) void hsv_apply_kernel(const T* __restrict__ images, O* __restrict__ out, HsvArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
#pragma clang fp contract(off)      // (every fused multiply-add below is written out: the pack and the single-pixel forms give the same bits)
    static_assert(!(kInter && kMask), "the masked forms are planar");
    constexpr int TPB = kStreamThreads;
    __shared__ float row[6];      // (the last word says whether the tile is copied through)
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const uint8_t* msk = tile_mask(mk, tile, a.pixels);
    const int64_t p_begin = (int64_t)chunk_id * a.chunk;
    const int64_t p_end = min(p_begin + (int64_t)a.chunk, a.pixels);
    const T* img = images + tile * 3 * a.pixels;
    O* dst = out + tile * 3 * a.pixels;

    int64_t p = p_begin + (int64_t)threadIdx.x * V;
    float u[3][V];
    MaskPack<V> mp;
    mp.clear();
    if (p < p_end) {
        deconv_load<T, V, kInter>(img, a.pixels, p, u);
        if constexpr (kMask) mp.load(msk + p);
    }

    if (threadIdx.x == 0) {
        const float* src = a.rows + (a.per_row ? tile * 5 : 0);
        constexpr float kInf = __builtin_huge_valf();
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float v = src[i];
            row[i] = v;
            finite = finite && fabsf(v) < kInf;      // (false for a NaN)
        }
        row[5] = finite ? 0.0f : 1.0f;
    }
    __syncthreads();
    auto uniform = [&](int i) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(row[i]))); };
    const float shift = 6.0f * uniform(0), a_s = uniform(1), b_s = uniform(2), a_v = uniform(3), b_v255 = 255.0f * uniform(4);
    const bool through = uniform(5) != 0.0f;

    __shared__ uint4 stage[(kInter && V > 1 && sizeof(O) * V == 16) ? kStreamThreads * 3 : 1];      // 3 KB per wave: store_pixels_staged()
    while (p < p_end) {
        O res[3][V];
        uint32_t in_bits = ~0u;
        if constexpr (kMask) in_bits = mp.bits();
        if (through) in_bits = 0u;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float lr = input_level<T>(u[0][i]), lg = input_level<T>(u[1][i]), lb = input_level<T>(u[2][i]);
            const bool copy = !in_mask(in_bits, i) || lr != lr || lg != lg || lb != lb;
            float r = lr, g = lg, b = lb;
            if constexpr (sizeof(T) != 1) {      // (a byte is a level already)
                r = fminf(fmaxf(lr, 0.0f), 255.0f);
                g = fminf(fmaxf(lg, 0.0f), 255.0f);
                b = fminf(fmaxf(lb, 0.0f), 255.0f);
            }
            const float hi = fmaxf(r, fmaxf(g, b)), lo = fminf(r, fminf(g, b)), c = hi - lo;
            const float s = hi > 0.0f ? hsv_quotient<T>(c, hi) : 0.0f;
            // (one quotient: the numerator and the sector's offset are selected first; C == 0 is M == r with h6 = 0.  h6 lies in (-1, 6): the
            // "+ 6 if negative" of the rule is done by the reduction below, which wraps a negative sum as well)
            const float num = hi == r ? g - b : (hi == g ? b - r : r - g);
            const float sector = hi == r ? 0.0f : (hi == g ? 2.0f : 4.0f);
            const float h6 = sector + (c > 0.0f ? hsv_quotient<T>(num, c) : 0.0f);
            float h = h6 + shift;
            h = fmaf(-6.0f, floorf(h * (1.0f / 6.0f)), h);
            h = h < 0.0f ? h + 6.0f : h;      // (the product with the rounded 1 / 6 may reach the next integer just below a multiple of 6; [0, 6] after this)
            const float s2 = fminf(fmaxf(fmaf(a_s, s, b_s), 0.0f), 1.0f);
            const float v2 = fminf(fmaxf(fmaf(a_v, hi, b_v255), 0.0f), 255.0f);      // 255 clamp(a_v M / 255 + b_v, 0, 1), without the quotient: the identity row gives M itself
            const float vs = v2 * s2;
            // t of the rule without the wrap of k: for r (n = 5) min(k, 4 - k) is 2 - |h - 3| where it is positive, for g (n = 3) and b (n = 1)
            // it is |h - 2| - 1 and |h - 4| - 1 where it is below 1 -- the same piecewise-linear functions of h on [0, 6], continuous at both ends
            const float t[3] = {fminf(fmaxf(2.0f - fabsf(h - 3.0f), 0.0f), 1.0f), fminf(fmaxf(fabsf(h - 2.0f) - 1.0f, 0.0f), 1.0f), fminf(fmaxf(fabsf(h - 4.0f) - 1.0f, 0.0f), 1.0f)};
            const float keep[3] = {r, g, b};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float level = fmaf(-vs, t[ch], v2);      // (in [0, V']: V' s' <= V' and t <= 1, and the fused result of a non-negative exact value is not negative)
                res[ch][i] = hsv_to_output<T, O, kUnit>(copy ? keep[ch] : level);
            }
        }
        const int64_t q = p;
        p += (int64_t)TPB * V;
        if (p < p_end) {      // (a work item of several pack sets: the next one is on its way while this one is stored)
            deconv_load<T, V, kInter>(img, a.pixels, p, u);
            if constexpr (kMask) mp.load(msk + p);
        }
        if constexpr (kInter && V > 1 && sizeof(O) * V == 16) {
            if (__builtin_amdgcn_ballot_w64(true) == ~0ull) {      // wave-uniform: every lane has a pack (all but a tile's last sweep)
                store_pixels_staged<O, V>(dst, q, res, stage + (threadIdx.x / kWave) * (3 * kWave));
                continue;
            }
        }
        store_pixels<O, V, kInter>(dst, a.pixels, q, res);
    }
}

// ---- host side: deconv_apply's pack rules (16 bytes of output per lane and plane; one pack set per work item on the vector paths, four
// for one-byte output, sixteen sweeps on the scalar path) ----
template <typename T, typename O, int V, bool kUnit, bool kInter, bool kMask = false>
static int run_hsv_apply(const T* images, O* out, HsvArgs a, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int VR = pack_for<O, V>();
    a.chunk = kStreamThreads * VR * (V == 1 ? 16 : apply_sets<O>());
    a.blocks = (int)((a.pixels + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL((hsv_apply_kernel<T, O, VR, kUnit, kInter, kMask>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, images, out, a, mk);
    return check_launch("hsv apply");
}

template <typename T, bool kMask = false>
static int hsv_apply_typed(const void* images, void* out, const HsvArgs& a, int out_code, bool interleaved, bool unit, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int W = PackOf<T>::n;
    bool vec = (a.pixels % W == 0) && aligned_for(images, 16) && aligned_for(out, out_elem_bytes(sizeof(T), out_code, unit) * W);
    if constexpr (kMask) vec = vec && aligned_for(mk.mask, W);      // (the mask's packs are as wide as the pixels': its pointer has a say of its own)
    const T* in = static_cast<const T*>(images);
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<W, kMask>(vec, interleaved, [&](auto v, auto inter) {
            return run_hsv_apply<T, O, decltype(v)::value, decltype(u)::value, decltype(inter)::value, kMask>(in, static_cast<O*>(out), a, stream, mk);
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
template <bool kMask>
static int hsv_apply_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, const unsigned char* mask_dev, unsigned flags,
                          void* stream_ptr) {
    const char* who = kMask ? "sx_hsv_apply_masked" : "sx_hsv_apply";
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    int rc = check_tiles(n, h, w);
    if (rc != SX_OK) return rc;
    if (!rows) return fail(SX_ERR_BAD_ARG, "rows pointer is null");
    if ((rc = check_rows("n_rows", n_rows, n)) != SX_OK) return rc;
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    rc = deconv_flags_ok(flags, dtype, kMask, who);
    if (rc != SX_OK) return rc;
    HsvArgs a{};
    a.rows = rows;
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_row = rows_per_tile(n_rows, n);
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return hsv_apply_typed<typename decltype(t)::type, kMask>(images, out, a, out_code, inter, unit, stream, mk); });
}

extern "C" int sx_hsv_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, unsigned flags, void* stream_ptr) {
    return hsv_apply_call<false>(images, out, dtype, n, h, w, rows, n_rows, nullptr, flags, stream_ptr);
}

extern "C" int sx_hsv_apply_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, const unsigned char* mask_dev,
                                   unsigned flags, void* stream_ptr) {
    return hsv_apply_call<true>(images, out, dtype, n, h, w, rows, n_rows, mask_dev, flags, stream_ptr);
}
