// Three-stain colour deconvolution with a GIVEN basis (Ruifrok & Johnston: HED, H-DAB, a complemented H&E estimate) -- included at the
// end of macenko.hip, whose streaming helpers it uses as they are: load_pack_stream, load_pixels, store_pixels, store_pixels_staged,
// LevelTables / l2_of, rgb_to_output, input_level, MaskArgs / MaskPack, kStreamThreads.  DESIGN.md 4n.
//
// A basis is 9 floats, (3, 3) row-major as [channel][stain] (columns are stain vectors, as HE's (3, 2)).  With the library's optical
// density OD_c = -ln((255 x_c + 1) / 240) = ln 240 - ln 2 * L_c (L_c the log2 level the parents' loops hold):
//   C = inverse(basis) OD,   C' = alpha * C + beta,   OD' = B_out C',   level_c = clamp(240 exp(-OD'_c), 0, 255)
// A 3x3 basis is invertible: nothing of the optical density is dropped, and combine(separate(x)) rebuilds x.
// Every call here is ONE launch: no workspace, no atomics, no traffic between workgroups, no waits.  Bases, factors and masks are device
// memory read by the kernel.  Per work item ONE thread inverts the basis in fp64 (closed form: adjugate x 1 / determinant -- a singular basis
// is not detected: Inf / NaN coefficients, which the clamp and the casts treat as the parents treat them), folds the whole map into a 3x3
// matrix plus an offset in the log2-level domain, rounds to float32 and hands the floats over through LDS, under the latency of the
// first pixel loads; the fold is read back wave-uniform (scalar registers).
namespace sx {
namespace macenko {

struct DeconvArgs {
    const float* basis;       // n_bases x 9: the source basis
    const float* target;      // n_targets x 9: B_out, or null: the source basis
    const float* alpha;       // N x 3 factors of the concentrations, or null (with beta): alpha = 1, beta = 0
    const float* beta;        // N x 3 shifts
    void* stains;             // separate: (3, N, 3, H, W) or (3, N, H, W, 3) of the output element, or null
    float* conc;              // separate: (N, 3, H, W) or (N, H, W, 3) float32, or null
    int64_t pixels, n_tiles;  // P = H*W, N
    int chunk, blocks;        // pixels per work item, work items per tile
    int per_basis, per_target;      // 1: row `tile`, 0: one row for the batch
};

// inverse(basis) in fp64, [stain][channel]: the adjugate over the determinant (its reciprocal: the hardware's v_rcp_f64 seed and two
// Newton steps, ~1e-15 relative, as pinv_of_he() -- the software fp64 division costs ~40 instructions and their registers on the one
// lane that runs this)
__device__ __forceinline__ void deconv_inverse(const float* __restrict__ b, double (&inv)[9]) {
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (double)b[i];
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    double r = __builtin_amdgcn_rcp(det);
    r = r * (2.0 - det * r);
    r = r * (2.0 - det * r);
    inv[0] = c00 * r;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) * r;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    inv[3] = c01 * r;
    inv[4] = (m[0] * m[8] - m[2] * m[6]) * r;
    inv[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    inv[6] = c02 * r;
    inv[7] = (m[1] * m[6] - m[0] * m[7]) * r;
    inv[8] = (m[0] * m[4] - m[1] * m[3]) * r;
}

// The map of one tile as twelve floats, apply_kernel's fold with three factors:
//   M[c][j] = sum_s B_out[c][s] alpha_s inv[s][j],   k[c] = log2(240) (1 - sum_j M[c][j]) - log2(e) sum_s B_out[c][s] beta_s,
//   level_c = 2^(sum_j M[c][j] L_j + k[c])
// (the row sum is taken over the ROUNDED coefficients, as in apply_kernel: a pixel of zero optical density, L_j = log2(240), then gets
// the offset's own level whatever the rounding of M did).
// The stain images of deconv_separate_kernel are this very function with alpha = e_i, beta = 0: the bits of deconv_apply_kernel.
// (B_out and the factors stay the floats they are until their row's turn: the inverse is the only fp64 array alive, so that the one
// lane's prologue does not set the kernel's register count)
__device__ __forceinline__ void deconv_fold(const float* __restrict__ bout, const double (&inv)[9], const float (&al)[3], const float (&be)[3], float* __restrict__ fold) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double b0 = (double)bout[c * 3], b1 = (double)bout[c * 3 + 1], b2 = (double)bout[c * 3 + 2];
        const double s0 = b0 * (double)al[0], s1 = b1 * (double)al[1], s2 = b2 * (double)al[2];
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = s0 * inv[j] + s1 * inv[3 + j] + s2 * inv[6 + j];
            const float mf = (float)v;
            fold[c * 3 + j] = mf;
            row += (double)mf;
        }
        fold[9 + c] = (float)(7.90689059560851852932 * (1.0 - row) - 1.44269504088896340736 * (b0 * (double)be[0] + b1 * (double)be[1] + b2 * (double)be[2]));      // log2(240), log2(e)
    }
}

__device__ __forceinline__ bool deconv_row_has_nan(const float* __restrict__ row) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) bad = bad || row[i] != row[i];
    return bad;
}

// The concentrations' twelve floats and their chain, ONE definition for the two kernels that hold concentrations (deconv_separate_kernel
// writes them, deconv_quantify_kernel bins them): a pixel's float32 concentrations are the same bits in both.
//   C_s = sum_j (-ln 2 inv[s][j]) L_j + ln 240 sum_j inv[s][j]
struct ConcFold {
    float ca[3][3], cb[3];
    // (the one lane's prologue) 9 + 3 floats from the fp64 inverse
    __device__ static __forceinline__ void fill(const double (&inv)[9], float* __restrict__ f) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) f[3 * s + j] = (float)(-0.69314718055994530942 * inv[3 * s + j]);      // ln 2
            f[9 + s] = (float)(5.48063892334199 * (inv[3 * s] + inv[3 * s + 1] + inv[3 * s + 2]));      // ln 240
        }
    }
    // (every lane, after the barrier) wave-uniform: scalar registers
    __device__ __forceinline__ void read(const float* __restrict__ f) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) ca[s][j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f[3 * s + j])));
            cb[s] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f[9 + s])));
        }
    }
    __device__ __forceinline__ float of(int s, float l0, float l1, float l2) const { return fmaf(ca[s][2], l2, fmaf(ca[s][1], l1, fmaf(ca[s][0], l0, cb[s]))); }
};

// The pixels of a pack set as the parents' loops take them: planar 16-byte packs non-temporally, everything else through load_pixels.
template <typename T, int V, bool kInter>
__device__ __forceinline__ void deconv_load(const T* __restrict__ img, int64_t pixels, int64_t p, float (&u)[3][V]) {
    if constexpr (!kInter && sizeof(T) * V == 16) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Pack<T, V> pk = load_pack_stream<T, V>(img + c * pixels + p);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if constexpr (sizeof(T) == 1) u[c][i] = __uint_as_float((uint32_t)pk.v[i]); else u[c][i] = raw_value<T>(pk.v[i]);
            }
        }
    } else {
        load_pixels<T, V, kInter, sizeof(T) == 1>(img, pixels, p, u);
    }
}

// sx_deconv_apply / sx_deconv_apply_masked: apply_kernel's shape with three factors.
// kMask (planar only): a masked-in pixel gets the arithmetic above, a masked-out pixel is copied (its input level through the same
// clamp, cast and / 255), and so is every pixel of a tile whose basis row -- or target row, if given -- holds a NaN.
template <typename T, typename O, int V, bool kUnit, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kStreamThreads) void deconv_apply_kernel(const T* __restrict__ images, O* __restrict__ out, DeconvArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    static_assert(!(kInter && kMask), "the masked forms are planar");
    constexpr int TPB = kStreamThreads;
    __shared__ LevelTables<T> tb;
    __shared__ float fold[kMask ? 13 : 12];      // (kMask: the last word says whether the tile is copied through)
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
        const float* b_src = a.basis + (a.per_basis ? tile * 9 : 0);
        const float* t_src = a.target ? a.target + (a.per_target ? tile * 9 : 0) : b_src;
        double inv[9];
        float al[3] = {1.0f, 1.0f, 1.0f}, be[3] = {0.0f, 0.0f, 0.0f};
        deconv_inverse(b_src, inv);
        if (a.alpha) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                al[s] = a.alpha[3 * tile + s];
                be[s] = a.beta[3 * tile + s];
            }
        }
        deconv_fold(t_src, inv, al, be, fold);
        if constexpr (kMask) fold[12] = (deconv_row_has_nan(b_src) || deconv_row_has_nan(t_src)) ? 1.0f : 0.0f;
    }
    tb.fill();
    __syncthreads();
    auto uniform = [&](int i) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fold[i]))); };
    float m[3][3], k[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < 3; ++j) m[c][j] = uniform(c * 3 + j);
        k[c] = uniform(9 + c);
    }
    bool through = false;
    if constexpr (kMask) through = fold[12] != 0.0f;

    __shared__ uint4 stage[(kInter && V > 1 && sizeof(O) * V == 16) ? kStreamThreads * 3 : 1];      // 3 KB per wave: store_pixels_staged()
    while (p < p_end) {
        O res[3][V];
        uint32_t in_bits = 0u;
        if constexpr (kMask) in_bits = through ? 0u : mp.bits();
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float l[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) l[c] = l2_of<T>(u[c][i], tb);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = fmaf(m[c][2], l[2], fmaf(m[c][1], l[1], fmaf(m[c][0], l[0], k[c])));
                if constexpr (kMask) {
                    const float rgb = in_mask(in_bits, i) ? __builtin_amdgcn_exp2f(x) : input_level<T>(u[c][i]);
                    res[c][i] = rgb_to_output<T, O, kUnit>(fminf(fmaxf(rgb, 0.0f), 255.0f));
                } else {
                    res[c][i] = rgb_to_output<T, O, kUnit>(fminf(fmaxf(__builtin_amdgcn_exp2f(x), 0.0f), 255.0f));
                }
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

// sx_deconv_separate: a pixel is read once; up to three stain images (9 planes) and three concentration maps are written.
// fold: 3 x 12 floats (stain image i: deconv_fold with alpha = e_i, beta = 0), then the concentrations' 9 + 3:
//   C_s = sum_j (-ln 2 inv[s][j]) L_j + ln 240 sum_j inv[s][j]
template <typename T, typename O, int V, bool kUnit, bool kInter>
__global__ __launch_bounds__(kStreamThreads) void deconv_separate_kernel(const T* __restrict__ images, DeconvArgs a) {
    constexpr int TPB = kStreamThreads;
    __shared__ LevelTables<T> tb;
    __shared__ float fold[48];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const int64_t p_begin = (int64_t)chunk_id * a.chunk;
    const int64_t p_end = min(p_begin + (int64_t)a.chunk, a.pixels);
    const T* img = images + tile * 3 * a.pixels;

    int64_t p = p_begin + (int64_t)threadIdx.x * V;
    float u[3][V];
    if (p < p_end) deconv_load<T, V, kInter>(img, a.pixels, p, u);

    if (threadIdx.x == 0) {
        const float* b_src = a.basis + (a.per_basis ? tile * 9 : 0);
        double inv[9];
        deconv_inverse(b_src, inv);
#pragma unroll 1
        for (int s = 0; s < 3; ++s) {
            const float al[3] = {s == 0 ? 1.0f : 0.0f, s == 1 ? 1.0f : 0.0f, s == 2 ? 1.0f : 0.0f}, be[3] = {0.0f, 0.0f, 0.0f};
            deconv_fold(b_src, inv, al, be, fold + 12 * s);
        }
        ConcFold::fill(inv, fold + 36);
    }
    tb.fill();
    __syncthreads();
    // (the fold is the same for every lane: read wave-uniform into scalar registers where it is used -- one stain's twelve floats at a
    // time, then the concentrations' twelve, not all 48 at once: that many live scalars spilled)
    auto uniform = [&](int i) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fold[i]))); };

    O* stains = static_cast<O*>(a.stains);
    float* conc = a.conc ? a.conc + tile * 3 * a.pixels : nullptr;

    __shared__ uint4 stage[(kInter && V > 1 && (sizeof(O) * V == 16 || V == 4)) ? kStreamThreads * 3 : 1];      // 3 KB per wave: store_pixels_staged()
    while (p < p_end) {
        float l[3][V];
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) l[c][i] = l2_of<T>(u[c][i], tb);
        const int64_t q = p;
        [[maybe_unused]] bool full = false;
        if constexpr (kInter && V > 1) full = __builtin_amdgcn_ballot_w64(true) == ~0ull;      // wave-uniform: every lane has a pack
        if (stains) {      // (uniform over the launch) the three images' packs, one after the other
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                float m[3][3], k[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) m[c][j] = uniform(12 * s + c * 3 + j);
                    k[c] = uniform(12 * s + 9 + c);
                }
                O res[3][V];
#pragma unroll
                for (int i = 0; i < V; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float x = fmaf(m[c][2], l[2][i], fmaf(m[c][1], l[1][i], fmaf(m[c][0], l[0][i], k[c])));
                        res[c][i] = rgb_to_output<T, O, kUnit>(fminf(fmaxf(__builtin_amdgcn_exp2f(x), 0.0f), 255.0f));
                    }
                O* dst = stains + ((int64_t)s * a.n_tiles + tile) * 3 * a.pixels;
                if constexpr (kInter && V > 1 && sizeof(O) * V == 16) {
                    if (full) {
                        store_pixels_staged<O, V>(dst, q, res, stage + (threadIdx.x / kWave) * (3 * kWave));
                        continue;
                    }
                }
                store_pixels<O, V, kInter>(dst, a.pixels, q, res);
            }
        }
        if (conc) {
            ConcFold cf;
            cf.read(fold + 36);
            float cc[3][V];
#pragma unroll
            for (int i = 0; i < V; ++i)
#pragma unroll
                for (int s = 0; s < 3; ++s) cc[s][i] = cf.of(s, l[0][i], l[1][i], l[2][i]);
            bool stored = false;
            if constexpr (kInter && V == 4) {      // (H, W, 3) float32 in 16-byte packs: the images' staged store
                if (full) {
                    store_pixels_staged<float, V>(conc, q, cc, stage + (threadIdx.x / kWave) * (3 * kWave));
                    stored = true;
                }
            }
            if (!stored) store_pixels<float, V, kInter>(conc, a.pixels, q, cc);
        }
        p += (int64_t)TPB * V;
        if (p < p_end) deconv_load<T, V, kInter>(img, a.pixels, p, u);      // (the scalar path's work items are sixteen sweeps; the vector paths' a single pack set)
    }
}

// sx_deconv_combine: three float32 concentration planes in, one image out: level_c = 2^(log2(240) - log2(e) sum_s basis[c][s] C_s).
template <typename O, int V, bool kUnit, bool kInter>
__global__ __launch_bounds__(kStreamThreads) void deconv_combine_kernel(const float* __restrict__ conc, O* __restrict__ out, DeconvArgs a) {
    constexpr int TPB = kStreamThreads;
    __shared__ float fold[9];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const int64_t p_begin = (int64_t)chunk_id * a.chunk;
    const int64_t p_end = min(p_begin + (int64_t)a.chunk, a.pixels);
    const float* src = conc + tile * 3 * a.pixels;
    O* dst = out + tile * 3 * a.pixels;

    int64_t p = p_begin + (int64_t)threadIdx.x * V;
    float cc[3][V];
    if (p < p_end) deconv_load<float, V, kInter>(src, a.pixels, p, cc);
    if (threadIdx.x < 9) fold[threadIdx.x] = (float)(-1.44269504088896340736 * (double)a.basis[(a.per_basis ? tile * 9 : 0) + threadIdx.x]);      // log2(e)
    __syncthreads();
    auto uniform = [&](int i) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fold[i]))); };
    float m[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int s = 0; s < 3; ++s) m[c][s] = uniform(c * 3 + s);
    const float k = 7.90689059560851852932f;      // log2(240)

    __shared__ uint4 stage[(kInter && V > 1 && sizeof(O) * V == 16) ? kStreamThreads * 3 : 1];
    while (p < p_end) {
        O res[3][V];
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = fmaf(m[c][2], cc[2][i], fmaf(m[c][1], cc[1][i], fmaf(m[c][0], cc[0][i], k)));
                res[c][i] = rgb_to_output<O, O, kUnit>(fminf(fmaxf(__builtin_amdgcn_exp2f(x), 0.0f), 255.0f));
            }
        const int64_t q = p;
        p += (int64_t)TPB * V;
        if (p < p_end) deconv_load<float, V, kInter>(src, a.pixels, p, cc);
        if constexpr (kInter && V > 1 && sizeof(O) * V == 16) {
            if (__builtin_amdgcn_ballot_w64(true) == ~0ull) {
                store_pixels_staged<O, V>(dst, q, res, stage + (threadIdx.x / kWave) * (3 * kWave));
                continue;
            }
        }
        store_pixels<O, V, kInter>(dst, a.pixels, q, res);
    }
}

// sx_deconv_quantify / sx_deconv_quantify_masked: 256-bin integer histograms of the three concentrations, their fixed-point sums and the
// number of counted pixels -- a pixel is read once and no map is written.  DESIGN.md 4o.
// The concentrations are deconv_separate_kernel's bits (ConcFold).  Binning is an exact function of them:
//   bin_s = clamp((int)floor(C_s 2^k) + z, 0, 255)      (the product with a power of two is exact)
//   term_s = C_s 2^16 converted to int32, round to nearest even, saturating; summed as int64
// A pixel counts iff its three concentrations are finite (and, kMask, its mask byte is set); a tile whose basis row holds a NaN counts
// nothing.  Integers throughout: the result does not depend on the order of the adds, it is the same run to run and adds up exactly
// over batches.
// A workgroup keeps kQuantCopies bank-striped copies of the 3 x 256 uint32 histogram in LDS (lane l adds into copy l % 16: the lanes
// of one ds_add_u32 that hit the SAME bin -- tissue clusters in a few bins -- spread over 16 addresses), the layout of
// histogram_masked_kernel in histmatch.hip.  A work item is kQuantPixels pixels of one tile, whatever the pack width: eight pack sets of
// float32, thirty-two sweeps of the scalar path.  Its flush -- 768 sums over the copies, a 64-bit global atomicAdd per NON-ZERO bin, three
// sums and one pixel count per wave -- is then a few percent of its adds.
constexpr int kQuantBins = 256;
constexpr int kQuantCopies = 16;
constexpr int kQuantPixels = 8192;                      // pixels per work item
constexpr int kQuantWords = 3 * kQuantBins + 3 + 1;     // a row of the output: [counts 3 x 256][sums 3][pixels 1]

struct QuantArgs {
    const float* basis;             // n_bases x 9
    unsigned long long* out;        // S x kQuantWords, zero when the kernel starts
    int64_t pixels, n_tiles;        // P = H*W, N
    int blocks;                     // work items per tile
    int per_basis, per_tile;        // 1: row `tile` of the bases / of the output, 0: row 0
    int zero_bin;                   // z
    float scale;                    // 2^k
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {      // (once per wave and stain: the shuffles' LDS round trips do not matter here)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;      // lane 0 holds the sum
}

template <typename T, int V, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kStreamThreads) void deconv_quantify_kernel(const T* __restrict__ images, QuantArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    static_assert(!(kInter && kMask), "the masked forms are planar");
    static_assert(kQuantPixels % (kStreamThreads * V) == 0, "a work item is a whole number of pack sets");
    constexpr int TPB = kStreamThreads;
    __shared__ LevelTables<T> tb;
    __shared__ float fold[13];      // (the last word: the tile's basis row holds a NaN)
    __shared__ __attribute__((aligned(16))) uint32_t hist[3 * kQuantBins * kQuantCopies];      // (16 bytes: cleared in uint4 stores)
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const uint8_t* msk = tile_mask(mk, tile, a.pixels);
    const int64_t p_begin = (int64_t)chunk_id * kQuantPixels;
    const int64_t p_end = min(p_begin + (int64_t)kQuantPixels, a.pixels);
    const T* img = images + tile * 3 * a.pixels;

    int64_t p = p_begin + (int64_t)threadIdx.x * V;
    float u[3][V];
    MaskPack<V> mp;
    mp.clear();
    if (p < p_end) {
        deconv_load<T, V, kInter>(img, a.pixels, p, u);
        if constexpr (kMask) mp.load(msk + p);
    }

    if (threadIdx.x == 0) {
        const float* b_src = a.basis + (a.per_basis ? tile * 9 : 0);
        double inv[9];
        deconv_inverse(b_src, inv);
        ConcFold::fill(inv, fold);
        fold[12] = deconv_row_has_nan(b_src) ? 1.0f : 0.0f;
    }
    {
        uint4* h4 = reinterpret_cast<uint4*>(hist);
        for (int i = threadIdx.x; i < 3 * kQuantBins * kQuantCopies / 4; i += TPB) h4[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    tb.fill();
    __syncthreads();
    if (fold[12] != 0.0f) return;      // (uniform over the workgroup; the output is zero already)
    ConcFold cf;
    cf.read(fold);
    const float scale = a.scale;
    const int zero_bin = a.zero_bin;
    uint32_t* mine = hist + (threadIdx.x & (kQuantCopies - 1));

    long long sum[3] = {0ll, 0ll, 0ll};
    uint32_t counted = 0u;      // wave-uniform: the wave's counted pixels
    while (p < p_end) {
        const int64_t p_next = p + (int64_t)TPB * V;
        const bool more = p_next < p_end;
        float un[3][V];
        MaskPack<V> mn;
        mn.clear();
        if (more) {      // (the next pack set is on its way while this one is counted)
            deconv_load<T, V, kInter>(img, a.pixels, p_next, un);
            if constexpr (kMask) mn.load(msk + p_next);
        }
        uint32_t in_bits = ~0u;
        if constexpr (kMask) in_bits = mp.bits();
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float l[3], c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k] = l2_of<T>(u[k][i], tb);
#pragma unroll
            for (int s = 0; s < 3; ++s) c[s] = cf.of(s, l[0], l[1], l[2]);
            constexpr float kInf = __builtin_huge_valf();
            const bool ok = in_mask(in_bits, i) && fabsf(c[0]) < kInf && fabsf(c[1]) < kInf && fabsf(c[2]) < kInf;
            counted += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ok));
            if (ok) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float f = fminf(fmaxf(floorf(c[s] * scale), -1024.0f), 1024.0f);      // (beyond every bin either way: the int conversion stays defined)
                    const int bin = min(max((int)f + zero_bin, 0), kQuantBins - 1);
                    atomicAdd(&mine[(s * kQuantBins + bin) * kQuantCopies], 1u);
                    const float t = rintf(c[s] * 65536.0f);
                    const int term = t >= 2147483648.0f ? 2147483647 : (t <= -2147483648.0f ? (-2147483647 - 1) : (int)t);      // v_cvt_i32_f32's saturation, spelled out
                    sum[s] += (long long)term;
                }
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < V; ++i) u[k][i] = un[k][i];
            mp = mn;
        }
        p = p_next;
    }
    // (a thread without a pack never entered the loop: its ballots are missing from `counted`, which only lane 0 of a wave uses -- and
    // lane 0 holds the lowest pixel of its wave, so it ran every sweep any lane of its wave ran)
    __syncthreads();
    unsigned long long* row = a.out + (a.per_tile ? tile : 0) * kQuantWords;
    for (int i = threadIdx.x; i < 3 * kQuantBins; i += TPB) {      // thread t adds up the copies of its bins, starting at its own bank
        uint32_t total = 0u;
#pragma unroll
        for (int k = 0; k < kQuantCopies; ++k) total += hist[i * kQuantCopies + ((threadIdx.x + k) & (kQuantCopies - 1))];
        if (total) atomicAdd(&row[i], (unsigned long long)total);
    }
    const uint32_t wave_counted = (uint32_t)__builtin_amdgcn_readfirstlane((int)counted);
    if (wave_counted) {      // (wave-uniform)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const long long total = wave_sum_i64(sum[s]);
            if (lane_id() == 0 && total != 0ll) atomicAdd(&row[3 * kQuantBins + s], (unsigned long long)total);      // (two's complement: the 64-bit add is the signed add)
        }
        if (lane_id() == 0) atomicAdd(&row[3 * kQuantBins + 3], (unsigned long long)wave_counted);
    }
}

// sx_deconv_moments / sx_deconv_moments_masked: first and second moments of the three concentrations as integers -- quantify's loop and
// counting rule without the histogram.  DESIGN.md 4q.
//   t_s = quantify's term (C_s 2^16, round to nearest even, saturating to int32)      sums_s    += t_s
//   u_s = clamp(t_s, -2^22, 2^22)                                                     squares_s += (u_s u_s) >> 8      (unit 2^-24, floored)
// Seven int64 accumulators per lane, one shuffle reduction per wave and word, the waves' totals through 4 x 7 LDS words, then seven
// 64-bit global adds per WORKGROUP (non-zero totals only).  No LDS atomics, no table but the level tables.
constexpr int kMomentWords = 7;      // a row of the output: [sums 3][squares 3][pixels 1]
constexpr int kMomentClamp = 1 << 22;

struct MomentArgs {
    const float* basis;             // n_bases x 9
    unsigned long long* out;        // S x kMomentWords, zero when the kernel starts
    int64_t pixels, n_tiles;        // P = H*W, N
    int blocks;                     // work items per tile
    int per_basis, per_tile;        // 1: row `tile` of the bases / of the output, 0: row 0
};

template <typename T, int V, bool kInter, bool kMask = false>
__global__ __launch_bounds__(kStreamThreads) void deconv_moments_kernel(const T* __restrict__ images, MomentArgs a, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    static_assert(!(kInter && kMask), "the masked forms are planar");
    static_assert(kQuantPixels % (kStreamThreads * V) == 0, "a work item is a whole number of pack sets");
    constexpr int TPB = kStreamThreads;
    constexpr int kWaves = kStreamThreads / kWave;
    __shared__ LevelTables<T> tb;
    __shared__ float fold[13];      // (the last word: the tile's basis row holds a NaN)
    __shared__ long long red[kWaves][kMomentWords];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk_id = (int)(blockIdx.x % (unsigned)a.blocks);
    const uint8_t* msk = tile_mask(mk, tile, a.pixels);
    const int64_t p_begin = (int64_t)chunk_id * kQuantPixels;
    const int64_t p_end = min(p_begin + (int64_t)kQuantPixels, a.pixels);
    const T* img = images + tile * 3 * a.pixels;

    int64_t p = p_begin + (int64_t)threadIdx.x * V;
    float u[3][V];
    MaskPack<V> mp;
    mp.clear();
    if (p < p_end) {
        deconv_load<T, V, kInter>(img, a.pixels, p, u);
        if constexpr (kMask) mp.load(msk + p);
    }

    if (threadIdx.x == 0) {
        const float* b_src = a.basis + (a.per_basis ? tile * 9 : 0);
        double inv[9];
        deconv_inverse(b_src, inv);
        ConcFold::fill(inv, fold);
        fold[12] = deconv_row_has_nan(b_src) ? 1.0f : 0.0f;
    }
    tb.fill();
    __syncthreads();
    if (fold[12] != 0.0f) return;      // (uniform over the workgroup; the output is zero already)
    ConcFold cf;
    cf.read(fold);

    long long acc[kMomentWords] = {0ll, 0ll, 0ll, 0ll, 0ll, 0ll, 0ll};
    while (p < p_end) {
        const int64_t p_next = p + (int64_t)TPB * V;
        const bool more = p_next < p_end;
        float un[3][V];
        MaskPack<V> mn;
        mn.clear();
        if (more) {      // (the next pack set is on its way while this one is summed)
            deconv_load<T, V, kInter>(img, a.pixels, p_next, un);
            if constexpr (kMask) mn.load(msk + p_next);
        }
        uint32_t in_bits = ~0u;
        if constexpr (kMask) in_bits = mp.bits();
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float l[3], c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k] = l2_of<T>(u[k][i], tb);
#pragma unroll
            for (int s = 0; s < 3; ++s) c[s] = cf.of(s, l[0], l[1], l[2]);
            constexpr float kInf = __builtin_huge_valf();
            const bool ok = in_mask(in_bits, i) && fabsf(c[0]) < kInf && fabsf(c[1]) < kInf && fabsf(c[2]) < kInf;
            if (ok) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float t = rintf(c[s] * 65536.0f);
                    const int term = t >= 2147483648.0f ? 2147483647 : (t <= -2147483648.0f ? (-2147483647 - 1) : (int)t);      // v_cvt_i32_f32's saturation, spelled out
                    const long long uu = (long long)min(max(term, -kMomentClamp), kMomentClamp);
                    acc[s] += (long long)term;
                    acc[3 + s] += (uu * uu) >> 8;      // (at most 2^44 >> 8: non-negative, the shift is the floor)
                }
                acc[6] += 1ll;
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < V; ++i) u[k][i] = un[k][i];
            mp = mn;
        }
        p = p_next;
    }
    // (every thread arrives here: a thread without a pack holds zeros)
    // wave_sum_i64: 64-bit shuffles, two LDS round trips a step.  The DPP reductions of common.hpp are 32-bit; a 64-bit sum on them needs the
    // carry between the halves at every step.  Seven reductions per wave and WORK ITEM (8192 pixels), independent of each other; not timed on their own.
    const int wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < kMomentWords; ++k) {
        const long long total = wave_sum_i64(acc[k]);
        if (lane_id() == 0) red[wave][k] = total;
    }
    __syncthreads();
    if (threadIdx.x < kMomentWords) {
        long long total = 0ll;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) total += red[wv][threadIdx.x];
        unsigned long long* row = a.out + (a.per_tile ? tile : 0) * kMomentWords;
        if (total != 0ll) atomicAdd(&row[threadIdx.x], (unsigned long long)total);      // (two's complement: the 64-bit add is the signed add)
    }
}

// ---- host side: the parents' pack rules (16 bytes of output per lane and plane: VR; one pack set per work item on the vector paths,
// four for one-byte output, sixteen sweeps on the scalar path) ----
template <typename T, typename O, int V, bool kUnit, bool kInter, bool kMask = false>
static int run_deconv_apply(const T* images, O* out, DeconvArgs a, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int VR = pack_for<O, V>();
    a.chunk = kStreamThreads * VR * (V == 1 ? 16 : apply_sets<O>());
    a.blocks = (int)((a.pixels + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL((deconv_apply_kernel<T, O, VR, kUnit, kInter, kMask>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, images, out, a, mk);
    return check_launch("deconv apply");
}

template <typename T, bool kMask = false>
static int deconv_apply_typed(const void* images, void* out, const DeconvArgs& a, int out_code, bool interleaved, bool unit, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int W = PackOf<T>::n;
    bool vec = (a.pixels % W == 0) && aligned_for(images, 16) && aligned_for(out, out_elem_bytes(sizeof(T), out_code, unit) * W);
    if constexpr (kMask) vec = vec && aligned_for(mk.mask, W);      // (the mask's packs are as wide as the pixels': its pointer has a say of its own)
    const T* in = static_cast<const T*>(images);
    return with_out<T>(out_code, unit, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<W, kMask>(vec, interleaved, [&](auto v, auto inter) {
            return run_deconv_apply<T, O, decltype(v)::value, decltype(u)::value, decltype(inter)::value, kMask>(in, static_cast<O*>(out), a, stream, mk);
        });
    });
}

template <typename T, typename O, int V, bool kUnit, bool kInter>
static int run_deconv_separate(const T* images, DeconvArgs a, hipStream_t stream) {
    constexpr int VR = pack_for<O, V>();
    a.chunk = kStreamThreads * VR * (VR == 1 ? 16 : 1);
    a.blocks = (int)((a.pixels + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL((deconv_separate_kernel<T, O, VR, kUnit, kInter>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, images, a);
    return check_launch("deconv separate");
}

template <typename T>
static int deconv_separate_typed(const void* images, const DeconvArgs& a, int out_code, bool interleaved, bool unit, hipStream_t stream) {
    const bool stains = a.stains != nullptr;
    constexpr int W = PackOf<T>::n;
    const bool vec = (a.pixels % W == 0) && aligned_for(images, 16) && (!stains || aligned_for(a.stains, out_elem_bytes(sizeof(T), out_code, unit) * W)) && (!a.conc || aligned_for(a.conc, 16));
    const T* in = static_cast<const T*>(images);
    // (O: the images' element -- float for a call without images)
    return with_out<T>(out_code, unit, stains, [&](auto o, auto u) {
        using O = typename decltype(o)::type;
        return with_layout<W>(vec, interleaved, [&](auto v, auto inter) {
            return run_deconv_separate<T, O, decltype(v)::value, decltype(u)::value, decltype(inter)::value>(in, a, stream);
        });
    });
}

// (two pack widths: four float32 concentrations per plane and lane where the pointers and the tile size allow it, single pixels otherwise)
template <typename O, bool kUnit>
static int deconv_combine_typed(const float* conc, void* out, DeconvArgs a, bool interleaved, hipStream_t stream) {
    const bool vec = (a.pixels % 4 == 0) && aligned_for(conc, 16) && aligned_for(out, sizeof(O) * 4);
    a.chunk = kStreamThreads * (vec ? 4 * apply_sets<O>() : 16);
    a.blocks = (int)((a.pixels + a.chunk - 1) / a.chunk);
    const dim3 grid((unsigned)(a.n_tiles * a.blocks)), block(kStreamThreads);
    O* dst = static_cast<O*>(out);
    return with_layout<4>(vec, interleaved, [&](auto v, auto inter) {
        hipLaunchKernelGGL((deconv_combine_kernel<O, decltype(v)::value, kUnit, decltype(inter)::value>), grid, block, 0, stream, conc, dst, a);
        return check_launch("deconv combine");
    });
}

template <typename T, int V, bool kInter, bool kMask = false>
static int run_deconv_quantify(const T* images, QuantArgs a, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    a.blocks = (int)((a.pixels + kQuantPixels - 1) / kQuantPixels);
    hipLaunchKernelGGL((deconv_quantify_kernel<T, V, kInter, kMask>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, images, a, mk);
    return check_launch("deconv quantify");
}

// (the siblings' pack rule: 16-byte packs where the tile size and the image pointer allow it -- and, masked, the mask pointer, whose packs
// are as wide as the pixels' --, single pixels otherwise)
template <typename T, bool kMask = false>
static int deconv_quantify_typed(const void* images, const QuantArgs& a, bool interleaved, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int W = PackOf<T>::n;
    bool vec = (a.pixels % W == 0) && aligned_for(images, 16);
    const T* in = static_cast<const T*>(images);
    if constexpr (kMask) vec = vec && aligned_for(mk.mask, W);
    return with_layout<W, kMask>(vec, interleaved, [&](auto v, auto inter) { return run_deconv_quantify<T, decltype(v)::value, decltype(inter)::value, kMask>(in, a, stream, mk); });
}

// The zeroes of a call on a stream that is being CAPTURED: a clearing launch instead of the memset.  (What a memset node of a captured
// graph writes on replay depends, with HIP 7.0 / ROCm 7.2 on gfx950, on what was launched since the previous replay: tools/probe_graph_memset.py,
// profiles/graph_memset_probe.txt.  A kernel node replays its own arguments.  DESIGN.md 4q.)
__global__ void moments_clear_kernel(unsigned long long* __restrict__ out, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) out[i] = 0ull;
}

// (quantify's work items and pack rule)
template <typename T, bool kMask = false>
static int deconv_moments_typed(const void* images, MomentArgs a, bool interleaved, hipStream_t stream, MaskArgs<kMask> mk = MaskArgs<kMask>{}) {
    constexpr int W = PackOf<T>::n;
    bool vec = (a.pixels % W == 0) && aligned_for(images, 16);
    const T* in = static_cast<const T*>(images);
    if constexpr (kMask) vec = vec && aligned_for(mk.mask, W);
    a.blocks = (int)((a.pixels + kQuantPixels - 1) / kQuantPixels);
    return with_layout<W, kMask>(vec, interleaved, [&](auto v, auto inter) {
        hipLaunchKernelGGL((deconv_moments_kernel<T, decltype(v)::value, decltype(inter)::value, kMask>), dim3((unsigned)(a.n_tiles * a.blocks)), dim3(kStreamThreads), 0, stream, in, a, mk);
        return check_launch("deconv moments");
    });
}

}  // namespace macenko
}  // namespace sx

// ---- C ABI (include/stainx_hip.h) ----
static int deconv_common_ok(const void* images, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, const char* what) {
    if (!images) return fail(SX_ERR_BAD_ARG, "%s pointer is null", what);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "tiles must have positive sizes, got N=%lld H=%lld W=%lld", (long long)n, (long long)h, (long long)w);
    if (n * h * w >= (1ll << 32)) return fail(SX_ERR_BAD_ARG, "N*H*W must be below 2^32 pixels");
    if (!basis) return fail(SX_ERR_BAD_ARG, "basis pointer is null");
    if (n_bases != 1 && n_bases != n) return fail(SX_ERR_BAD_ARG, "n_bases must be 1 (one basis for the batch) or n_tiles = %lld, got %lld", (long long)n, (long long)n_bases);
    return SX_OK;
}

static int deconv_flags_ok(unsigned flags, int dtype, bool planar_only, const char* who) {
    const unsigned allowed = SX_MACENKO_NORMALIZE_0_1 | SX_MACENKO_CLASSIC | SX_MACENKO_OUT_BF16 | SX_MACENKO_OUT_F16 | (planar_only ? 0u : SX_MACENKO_CHANNELS_LAST);
    if (planar_only && (flags & SX_MACENKO_CHANNELS_LAST)) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes planar (N,3,H,W) tiles only (no SX_MACENKO_CHANNELS_LAST)", flags, who);
    if (flags & ~allowed) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes SX_MACENKO_NORMALIZE_0_1, _CHANNELS_LAST, _CLASSIC, _OUT_BF16 and _OUT_F16 only", flags, who);
    return out_flags_ok(flags, dtype);
}

template <bool kMask>
static int deconv_apply_call(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, const float* target, int64_t n_targets,
                             const float* alpha, const float* beta, const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    const char* who = kMask ? "sx_deconv_apply_masked" : "sx_deconv_apply";
    int rc = deconv_common_ok(images, n, h, w, basis, n_bases, "images");
    if (rc != SX_OK) return rc;
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    if (target && n_targets != 1 && n_targets != n) return fail(SX_ERR_BAD_ARG, "n_targets must be 1 (one target basis for the batch) or n_tiles = %lld, got %lld", (long long)n, (long long)n_targets);
    if ((alpha == nullptr) != (beta == nullptr)) return fail(SX_ERR_BAD_ARG, "alpha and beta: both given or both null");
    rc = deconv_flags_ok(flags, dtype, kMask, who);
    if (rc != SX_OK) return rc;
    DeconvArgs a{};
    a.basis = basis;
    a.target = target;
    a.alpha = alpha;
    a.beta = beta;
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_basis = n_bases == n && n != 1 ? 1 : 0;
    a.per_target = target && n_targets == n && n != 1 ? 1 : 0;
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return deconv_apply_typed<typename decltype(t)::type, kMask>(images, out, a, out_code, inter, unit, stream, mk); });
}

extern "C" int sx_deconv_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, const float* target, int64_t n_targets,
                               const float* alpha, const float* beta, unsigned flags, void* stream_ptr) {
    return deconv_apply_call<false>(images, out, dtype, n, h, w, basis, n_bases, target, n_targets, alpha, beta, nullptr, flags, stream_ptr);
}

extern "C" int sx_deconv_apply_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, const float* target, int64_t n_targets,
                                      const float* alpha, const float* beta, const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    return deconv_apply_call<true>(images, out, dtype, n, h, w, basis, n_bases, target, n_targets, alpha, beta, mask_dev, flags, stream_ptr);
}

extern "C" int sx_deconv_separate(const void* images, void* stains_out, float* conc_out, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, unsigned flags,
                                  void* stream_ptr) {
    int rc = deconv_common_ok(images, n, h, w, basis, n_bases, "images");
    if (rc != SX_OK) return rc;
    if (!stains_out && !conc_out) return fail(SX_ERR_BAD_ARG, "stains_out and conc_out are both null: nothing to separate into");
    rc = deconv_flags_ok(flags, dtype, false, "sx_deconv_separate");
    if (rc != SX_OK) return rc;
    DeconvArgs a{};
    a.basis = basis;
    a.stains = stains_out;
    a.conc = conc_out;
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_basis = n_bases == n && n != 1 ? 1 : 0;
    const int out_code = out_code_of(flags);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return deconv_separate_typed<typename decltype(t)::type>(images, a, out_code, inter, unit, stream); });
}

extern "C" int sx_deconv_combine(const float* conc, void* out, int out_dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, unsigned flags, void* stream_ptr) {
    int rc = deconv_common_ok(conc, n, h, w, basis, n_bases, "concentrations");
    if (rc != SX_OK) return rc;
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    if (flags & ~(SX_MACENKO_NORMALIZE_0_1 | SX_MACENKO_CHANNELS_LAST | SX_MACENKO_CLASSIC))
        return fail(SX_ERR_BAD_ARG, "flags 0x%x: sx_deconv_combine takes SX_MACENKO_NORMALIZE_0_1, _CHANNELS_LAST and _CLASSIC only (the output element is out_dtype)", flags);
    const bool unit = (flags & SX_MACENKO_NORMALIZE_0_1) != 0;
    if (unit && out_dtype == SX_U8) return fail(SX_ERR_BAD_ARG, "SX_MACENKO_NORMALIZE_0_1 with uint8 output: / 255 is fused for float outputs only");
    DeconvArgs a{};
    a.basis = basis;
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_basis = n_bases == n && n != 1 ? 1 : 0;
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    // (the output's element; uint8 has no fused / 255: refused above)
    return with_dtype(out_dtype, [&](auto t) {
        using O = typename decltype(t)::type;
        if constexpr (sizeof(O) == 1) return deconv_combine_typed<O, false>(conc, out, a, inter, stream);
        else return unit ? deconv_combine_typed<O, true>(conc, out, a, inter, stream) : deconv_combine_typed<O, false>(conc, out, a, inter, stream);
    });
}

template <bool kMask>
static int deconv_quantify_call(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int bin_log2, int zero_bin, int per_tile,
                                long long* out, const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    const char* who = kMask ? "sx_deconv_quantify_masked" : "sx_deconv_quantify";
    int rc = deconv_common_ok(images, n, h, w, basis, n_bases, "images");
    if (rc != SX_OK) return rc;
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    if (bin_log2 < 0 || bin_log2 > 8) return fail(SX_ERR_BAD_ARG, "bin_log2 must lie in [0, 8] (bins of width 2^-bin_log2), got %d", bin_log2);
    if (zero_bin < 0 || zero_bin > 255) return fail(SX_ERR_BAD_ARG, "zero_bin must lie in [0, 255] (the bin whose lower edge is concentration 0), got %d", zero_bin);
    if (kMask && (flags & SX_MACENKO_CHANNELS_LAST)) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes planar (N,3,H,W) tiles only (no SX_MACENKO_CHANNELS_LAST)", flags, who);
    if (flags & ~(SX_MACENKO_CHANNELS_LAST | SX_MACENKO_CLASSIC)) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes SX_MACENKO_CHANNELS_LAST and SX_MACENKO_CLASSIC only (there is no output image)", flags, who);
    QuantArgs a{};
    a.basis = basis;
    a.out = reinterpret_cast<unsigned long long*>(out);
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_basis = n_bases == n && n != 1 ? 1 : 0;
    a.per_tile = per_tile ? 1 : 0;
    a.zero_bin = zero_bin;
    a.scale = (float)(1 << bin_log2);
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if ((rc = dtype_ok(dtype)) != SX_OK) return rc;      // (before anything is enqueued)
    const size_t bytes = (size_t)(per_tile ? n : 1) * kQuantWords * sizeof(unsigned long long);
    if (hipMemsetAsync(out, 0, bytes, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return deconv_quantify_typed<typename decltype(t)::type, kMask>(images, a, inter, stream, mk); });
}

extern "C" int sx_deconv_quantify(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int bin_log2, int zero_bin, int per_tile,
                                  long long* out, unsigned flags, void* stream_ptr) {
    return deconv_quantify_call<false>(images, dtype, n, h, w, basis, n_bases, bin_log2, zero_bin, per_tile, out, nullptr, flags, stream_ptr);
}

extern "C" int sx_deconv_quantify_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int bin_log2, int zero_bin, int per_tile,
                                         long long* out, const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    return deconv_quantify_call<true>(images, dtype, n, h, w, basis, n_bases, bin_log2, zero_bin, per_tile, out, mask_dev, flags, stream_ptr);
}

template <bool kMask>
static int deconv_moments_call(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int per_tile, long long* out,
                               const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    const char* who = kMask ? "sx_deconv_moments_masked" : "sx_deconv_moments";
    int rc = deconv_common_ok(images, n, h, w, basis, n_bases, "images");
    if (rc != SX_OK) return rc;
    if (!out) return fail(SX_ERR_BAD_ARG, "out pointer is null");
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    if (kMask && (flags & SX_MACENKO_CHANNELS_LAST)) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes planar (N,3,H,W) tiles only (no SX_MACENKO_CHANNELS_LAST)", flags, who);
    if (flags & ~(SX_MACENKO_CHANNELS_LAST | SX_MACENKO_CLASSIC)) return fail(SX_ERR_BAD_ARG, "flags 0x%x: %s takes SX_MACENKO_CHANNELS_LAST and SX_MACENKO_CLASSIC only (there is no output image)", flags, who);
    MomentArgs a{};
    a.basis = basis;
    a.out = reinterpret_cast<unsigned long long*>(out);
    a.pixels = h * w;
    a.n_tiles = n;
    a.per_basis = n_bases == n && n != 1 ? 1 : 0;
    a.per_tile = per_tile ? 1 : 0;
    const bool inter = (flags & SX_MACENKO_CHANNELS_LAST) != 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    if ((rc = dtype_ok(dtype)) != SX_OK) return rc;      // (before anything is enqueued)
    const int64_t words = (per_tile ? n : 1) * (int64_t)kMomentWords;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipStreamIsCapturing failed");
    if (capture == hipStreamCaptureStatusNone) {
        if (hipMemsetAsync(out, 0, (size_t)words * sizeof(unsigned long long), stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    } else {      // (see moments_clear_kernel)
        hipLaunchKernelGGL(moments_clear_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a.out, words);
        if ((rc = check_launch("deconv moments (clear)")) != SX_OK) return rc;
    }
    MaskArgs<kMask> mk{};
    if constexpr (kMask) mk.mask = mask_dev;
    return with_dtype(dtype, [&](auto t) { return deconv_moments_typed<typename decltype(t)::type, kMask>(images, a, inter, stream, mk); });
}

extern "C" int sx_deconv_moments(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int per_tile, long long* out, unsigned flags,
                                 void* stream_ptr) {
    return deconv_moments_call<false>(images, dtype, n, h, w, basis, n_bases, per_tile, out, nullptr, flags, stream_ptr);
}

extern "C" int sx_deconv_moments_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, const float* basis, int64_t n_bases, int per_tile, long long* out,
                                        const unsigned char* mask_dev, unsigned flags, void* stream_ptr) {
    return deconv_moments_call<true>(images, dtype, n, h, w, basis, n_bases, per_tile, out, mask_dev, flags, stream_ptr);
}
