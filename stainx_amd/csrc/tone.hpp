// Tone jitter: per-tile brightness, contrast, gamma and additive Gaussian noise (sx_tone_apply / sx_tone_apply_masked) -- included at the
// end of macenko.hip next to hsv.hpp, whose kernel shape, output rule (hsv_to_output) and copies it takes as they are, on the same streaming
// helpers: deconv_load / load_pixels, store_pixels, store_pixels_staged, MaskArgs / MaskPack / tile_mask, input_level, kStreamThreads.
// DESIGN.md 4v.  (The grey statistics that give a contrast change its pivot need the grey level of focus.hpp: tone_statistics.hpp, in
// reinhard.hip's translation unit.)
//
// A row is 4 floats (a, b, gamma, sigma).  All arithmetic is float32 on 0-255 levels; x is the input level (input_level<T>) clamped to
// [0, 255].  Per channel:
//   1. t = clamp(a x + 255 b, 0, 255)                                 one fused multiply-add; (1, 0) gives x exactly
//   2. gamma != 1:  t = 255 (t / 255)^gamma, 0 stays 0               a select on gamma == 1, not an evaluation
//   3. noise on:    t = clamp(t + 255 sigma z, 0, 255)                z a standard normal of (seed, pixel, channel)
// How the three steps are evaluated (what DESIGN.md 4v derives the error band from):
//   1. 255 b is held as the float32 pair (hi, lo), hi = fl(255 b), lo = fma(255, b, -hi) EXACTLY: t = fl(fl(a x + hi) + lo).  Where a x and
//      255 b cancel, the fused sum is exact or nearly so and lo restores what rounding 255 b took: the error of t is relative to t, which is
//      what a power below 1 needs next to 0.
//   2. 255 exp2f(gamma log2f(t (1 / 255))): the math library's log2f and exp2f, one unit in the last place each.
//   3. Philox4x32-10 with the pixel's index in the tile as the counter and the tile's seed as the key; four words -> four uniforms
//      u(w) = (2 (w >> 9) + 1) 2^-24 (exact, strictly inside (0, 1)) -> Box-Muller: rho = sqrtf(-2 logf(u(w0))), z_r = rho cospi(2 u(w1)),
//      z_g = rho sinpi(2 u(w1)); (w2, w3) the same way: z_b (cosine), z_s (sine).  sincospif takes the angle in half turns: 2 u is exact, no
//      product with pi is rounded.  shared_noise: all three channels get z_s.  The field is a function of (seed, pixel index) alone.
//
// Copies (hsv.hpp's, bit for bit): a pixel with a NaN in any channel, a masked-out pixel, and every pixel of a tile whose row has a
// non-finite member, gamma <= 0 or sigma < 0.  Every use of a value that may be NaN is a select.
//
// ONE launch per call: no workspace, no atomics, no memset; LDS holds the row, the seed and the staging area of the interleaved stores.
// kNoise = false (seeds == NULL) compiles without the generator: brightness / contrast / gamma alone is a plain stream.
namespace sx {
namespace macenko {

struct ToneArgs {
    const float* rows;           // n_rows x 4: (a, b, gamma, sigma)
    const long long* seeds;      // n_tiles, or null: no noise
    int64_t pixels, n_tiles;     // P = H*W, N
    int chunk, blocks;           // pixels per work item, work items per tile
    int per_row;                 // 1: row `tile`, 0: one row for the batch
    int shared_noise;            // 1: one normal per pixel for the three channels
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(kM0, c[0]), lo0 = kM0 * c[0], hi1 = __umulhi(kM1, c[2]), lo1 = kM1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
}

// Philox4x32-10 (Salmon et al. 2011; Random123's known answers: tests/test_tone_cpu.py): counter (c0, c1, 0, 0), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
    w[0] = c0, w[1] = c1, w[2] = 0u, w[3] = 0u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        philox_round(w, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ float tone_uniform(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 5.9604644775390625e-08f; }      // (an odd integer below 2^24, times 2^-24: exact)

// rho (cos, sin)(2 pi u1) of two words
__device__ __forceinline__ void tone_normals(uint32_t w0, uint32_t w1, float& z_cos, float& z_sin) {
#pragma clang fp contract(off)
    const float rho = sqrtf(-2.0f * logf(tone_uniform(w0)));
    float s, c;
    sincospif(2.0f * tone_uniform(w1), &s, &c);
    z_cos = rho * c;
    z_sin = rho * s;
}

template <typename T, typename O, int V, bool kUnit, bool kInter, bool kNoise, bool kMask = false>
__global__ __launch_bounds__(kStreamThreads) void tone_apply_kernel(const T* __restrict__ images, O* __restrict__ out, ToneArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
#pragma clang fp contract(off)      // (every fused multiply-add below is written out: the pack and the single-pixel forms give the same bits)
    static_assert(!(kInter && kMask), "the masked forms are planar");
    constexpr int TPB = kStreamThreads;
    __shared__ float row[6];         // a, hi and lo of 255 b, gamma, 255 sigma, and whether the tile is copied through
    __shared__ uint32_t key[2];      // the tile's seed
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
        const float* src = a.rows + (a.per_row ? tile * 4 : 0);
        constexpr float kInf = __builtin_huge_valf();
        const float ra = src[0], rb = src[1], rg = src[2], rs = src[3];
        const bool ok = fabsf(ra) < kInf && fabsf(rb) < kInf && fabsf(rg) < kInf && fabsf(rs) < kInf && rg > 0.0f && rs >= 0.0f;      // (false for a NaN)
        const float hi = 255.0f * rb;
        row[0] = ra;
        row[1] = hi;
        row[2] = fmaf(255.0f, rb, -hi);      // (exact: the rounding error of a float32 product is a float32)
        row[3] = rg;
        row[4] = 255.0f * rs;
        row[5] = ok ? 0.0f : 1.0f;
        if constexpr (kNoise) {
            const unsigned long long s = (unsigned long long)a.seeds[tile];
            key[0] = (uint32_t)s;
            key[1] = (uint32_t)(s >> 32);
        }
    }
    __syncthreads();
    auto uniform = [&](int i) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(row[i]))); };
    const float ta = uniform(0), b_hi = uniform(1), b_lo = uniform(2), gamma = uniform(3), s255 = uniform(4);
    const bool through = uniform(5) != 0.0f;
    const bool curved = gamma != 1.0f;
    [[maybe_unused]] uint32_t k0 = 0u, k1 = 0u;
    [[maybe_unused]] bool noisy = false;
    if constexpr (kNoise) {
        k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key[0]);
        k1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key[1]);
        noisy = s255 > 0.0f && !through;      // (a tile with sigma == 0 adds nothing: the generator does not run for it)
    }

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
            float keep[3] = {lr, lg, lb};
            if constexpr (sizeof(T) != 1) {      // (a byte is a level already)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) keep[ch] = fminf(fmaxf(keep[ch], 0.0f), 255.0f);
            }
            float z[3] = {0.0f, 0.0f, 0.0f};
            if constexpr (kNoise) {
                if (noisy) {      // (wave-uniform: the row is the tile's)
                    const uint64_t index = (uint64_t)(p + i);
                    uint32_t w[4];
                    philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), k0, k1, w);
                    float z_b, z_s;
                    tone_normals(w[2], w[3], z_b, z_s);
                    if (a.shared_noise) {      // (uniform over the launch)
                        z[0] = z[1] = z[2] = z_s;
                    } else {
                        tone_normals(w[0], w[1], z[0], z[1]);
                        z[2] = z_b;
                    }
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float t = fminf(fmaxf(fmaf(ta, keep[ch], b_hi) + b_lo, 0.0f), 255.0f);
                if (curved) {      // (wave-uniform)
                    const float powered = fminf(255.0f * exp2f(gamma * log2f(t * (1.0f / 255.0f))), 255.0f);
                    t = t > 0.0f ? powered : 0.0f;
                }
                if constexpr (kNoise) {
                    const float shaken = fminf(fmaxf(fmaf(s255, z[ch], t), 0.0f), 255.0f);
                    t = noisy ? shaken : t;
                }
                res[ch][i] = hsv_to_output<T, O, kUnit>(copy ? keep[ch] : t);
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

// ---- host side: hsv_apply's pack rules ----
template <typename T, typename O, int V, bool kUnit, bool kInter, bool kNoise, bool kMask = false>
static int run_tone_apply(const T* images, O* out, ToneArgs a, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int VR = pack_for<O, V>();
    a.chunk = kStreamThreads * VR * (V == 1 ? 16 : apply_sets<O>());
    a.blocks = (int)((a.pixels + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL((tone_apply_kernel<T, O, VR, kUnit, kInter, kNoise, kMask>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, images, out, a, mk);
    return check_launch("tone apply");
}

template <typename T, bool kMask = false>
static int tone_apply_typed(const void* images, void* out, const ToneArgs& a, int out_code, bool interleaved, bool unit, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int W = PackOf<T>::n;
    bool vec = (a.pixels % W == 0) && aligned_for(images, 16) && aligned_for(out, out_elem_bytes(sizeof(T), out_code, unit) * W);
    if constexpr (kMask) vec = vec && aligned_for(mk.mask, W);      // (the mask's packs are as wide as the pixels': its pointer has a say of its own)
    const T* in = static_cast<const T*>(images);
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<W, kMask>(vec, interleaved, [&](auto v, auto inter) {
            if (a.seeds) return run_tone_apply<T, O, decltype(v)::value, decltype(u)::value, decltype(inter)::value, true, kMask>(in, static_cast<O*>(out), a, stream, mk);
            return run_tone_apply<T, O, decltype(v)::value, decltype(u)::value, decltype(inter)::value, false, kMask>(in, static_cast<O*>(out), a, stream, mk);
        });
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
template <bool kMask>
static int tone_apply_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, const long long* seeds, int shared_noise,
                           const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    const char* who = kMask ? "sx_tone_apply_masked" : "sx_tone_apply";
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    int rc = check_tiles(n, h, w);
    if (rc != SX_OK) return rc;
    if (!rows) return fail(SX_ERR_BAD_ARG, "rows pointer is null");
    if ((rc = check_rows("n_rows", n_rows, n)) != SX_OK) return rc;
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    rc = deconv_flags_ok(flags, dtype, kMask, who);
    if (rc != SX_OK) return rc;
    ToneArgs a{};
    a.rows = rows;
    a.seeds = seeds;
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_row = rows_per_tile(n_rows, n);
    a.shared_noise = shared_noise != 0;
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return tone_apply_typed<typename decltype(t)::type, kMask>(images, out, a, out_code, inter, unit, stream, mk); });
}

extern "C" int sx_tone_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, const long long* seeds, int shared_noise,
                             unsigned flags, void* stream_ptr) {
    return tone_apply_call<false>(images, out, dtype, n, h, w, rows, n_rows, seeds, shared_noise, nullptr, flags, stream_ptr);
}

extern "C" int sx_tone_apply_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* rows, int64_t n_rows, const long long* seeds,
                                    int shared_noise, const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    return tone_apply_call<true>(images, out, dtype, n, h, w, rows, n_rows, seeds, shared_noise, mask_dev, flags, stream_ptr);
}
