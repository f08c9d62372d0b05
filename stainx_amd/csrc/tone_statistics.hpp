// Grey statistics (sx_grey_statistics / sx_grey_statistics_masked) -- included from reinhard.hip after focus.hpp, whose grey level
// (focus::grey_of: sx_grey_map's Y), streaming grid and clearing rule (focus::clear_words) the kernel here uses as they are.  DESIGN.md 4v.
//
// Per tile, or per batch, three int64 words: pixels, sum Y, sum Y^2 over the counted pixels -- HistoQC's brightness and RMS-contrast
// measures, and the pivot of a contrast change (stainx_amd.tone).  Every pixel is counted (a pixel with a NaN channel has Y = 0 and is
// counted); in the masked form only the pixels whose mask byte is non-zero.  The sums grey_map + level_histogram give, in ONE streaming
// launch that reads the tile once and writes no map.
//
// A lane keeps three 32-bit sums over a chunk of at most kGreyChunk sweeps (4 pixels a sweep at most: 65 536 pixels, and 65 536 x 255^2 is
// below 2^32: asserted), then the wave adds them up on the DPP path -- the count and sum Y as they are (64 lanes x 65 536 x 255 is below
// 2^32), sum Y^2 as its two 16-bit halves -- into wave-uniform 64-bit totals.  The waves' totals meet in LDS and the workgroup adds each
// word ONCE to the cleared output with a 64-bit integer add: integers only, independent of the order, poolable.
namespace sx {
namespace focus {

constexpr int kGreyWords = 3;           // a row of the output: pixels, sum Y, sum Y^2
constexpr int kGreyChunk = 16384;       // sweeps a lane adds up in 32 bits
constexpr int kGreyPooledGroups = 1024; // workgroups of a pooled call, about (see run_grey_statistics)
static_assert((unsigned long long)kGreyChunk * 4ull * 255ull * 255ull < (1ull << 32), "a lane's sum Y^2 of a chunk fits 32 bits");
static_assert((unsigned long long)kGreyChunk * 4ull * 255ull * kWave < (1ull << 32), "a wave's sum Y (and count) of a chunk fits 32 bits");

template <typename T, int V, bool kMask>
__global__ __launch_bounds__(kStreamThreads) void grey_statistics_kernel(const T* __restrict__ images, const uint8_t* __restrict__ mask, int64_t pixels, int channels_last, int blocks_per_tile,
                                                                         int pooled, unsigned long long* __restrict__ out) {
    static_assert(V == 1 || V == 4, "single pixels or packs of four");
    constexpr int kWaves = kStreamThreads / kWave;
    __shared__ unsigned long long parts[kWaves][kGreyWords];
    const int64_t tile = blockIdx.x / blocks_per_tile;
    const T* img = images + tile * 3 * pixels;
    const int64_t plane = channels_last ? 1 : pixels, step = channels_last ? 3 : 1;
    const int64_t stride = (int64_t)blocks_per_tile * kStreamThreads * V;
    unsigned long long total[kGreyWords] = {0ull, 0ull, 0ull};      // wave-uniform
    int64_t p = ((int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads + threadIdx.x) * V;
    // (the trip count of the outer loop is the workgroup's: every lane of a wave takes part in each reduction)
    for (int64_t first = (int64_t)(blockIdx.x % blocks_per_tile) * kStreamThreads * V; first < pixels; first += stride * kGreyChunk) {
        uint32_t count = 0, sum = 0, squares = 0;
        for (int k = 0; k < kGreyChunk && p < pixels; ++k, p += stride) {
            T v[3][V];
            detect::load_pixels<T, V>(img, p, pixels, step, plane, v);
            uint32_t in = ~0u;
            if constexpr (kMask) {
                if constexpr (V == 4) in = *reinterpret_cast<const uint32_t*>(mask + tile * pixels + p); else in = mask[tile * pixels + p];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const uint32_t y = grey_of<T>(v[0][i], v[1][i], v[2][i]);
                const bool counted = !kMask || ((in >> (8 * i)) & 0xFFu) != 0u;
                count += counted ? 1u : 0u;
                sum += counted ? y : 0u;
                squares += counted ? y * y : 0u;
            }
        }
        total[0] += wave_total_u32(count);
        total[1] += wave_total_u32(sum);
        total[2] += (unsigned long long)wave_total_u32(squares & 0xFFFFu) + ((unsigned long long)wave_total_u32(squares >> 16) << 16);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < kGreyWords; ++k) parts[threadIdx.x / kWave][k] = total[k];
    }
    __syncthreads();
    if (threadIdx.x < kGreyWords) {
        unsigned long long word = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) word += parts[k][threadIdx.x];
        if (word) atomicAdd(&out[(pooled ? 0 : tile) * kGreyWords + threadIdx.x], word);
    }
}

template <typename T, bool kMask>
static int run_grey_statistics(const void* images, const uint8_t* mask, int64_t n, int64_t pixels, int channels_last, int pooled, unsigned long long* out, hipStream_t stream) {
    bool vec = !channels_last && pixels % 4 == 0 && reinterpret_cast<uintptr_t>(images) % (sizeof(T) * 4) == 0;
    if (kMask) vec = vec && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
    int blocks_per_tile = saturation::level_blocks_per_tile(pixels, vec);
    // (pooled: every workgroup adds to the SAME three words, and the adds of one address are served one after the other -- with the per-tile
    // grid, 4096 workgroups for 64 tiles of 512 x 512, the pooled call took 56.8 us where the per-tile call takes 16.5.  About kGreyPooledGroups
    // workgroups, four a compute unit, stream as fast and add a quarter as often; the kernel's loop takes any share)
    if (pooled) blocks_per_tile = (int)std::max<int64_t>(1, std::min<int64_t>(blocks_per_tile, kGreyPooledGroups / n));
    const unsigned grid = (unsigned)(n * blocks_per_tile);
    if (vec)
        hipLaunchKernelGGL((grey_statistics_kernel<T, 4, kMask>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), mask, pixels, channels_last, blocks_per_tile, pooled, out);
    else
        hipLaunchKernelGGL((grey_statistics_kernel<T, 1, kMask>), dim3(grid), dim3(kStreamThreads), 0, stream, static_cast<const T*>(images), mask, pixels, channels_last, blocks_per_tile, pooled, out);
    return check_launch("grey statistics");
}

template <bool kMask>
static int grey_statistics_call(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int pooled, const unsigned char* mask_dev, long long* out, void* stream_ptr) {
    int rc;
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (!out) return fail(SX_ERR_BAD_ARG, "statistics_out pointer is null");
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "images must have positive sizes");
    if (kMask && (rc = check_mask(mask_dev)) != SX_OK) return rc;
    if (kMask && channels_last) return fail(SX_ERR_BAD_ARG, "sx_grey_statistics_masked takes planar (N,3,H,W) tiles only (channels_last must be 0)");
    if (n > 0x7fffffffll / detect::kBlocksPerTile) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    if ((rc = dtype_ok(dtype)) != SX_OK) return rc;      // (before anything is enqueued)
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(out);
    if ((rc = clear_words(words, (pooled ? 1 : n) * (int64_t)kGreyWords, stream)) != SX_OK) return rc;
    return with_dtype(dtype, [&](auto t) { return run_grey_statistics<typename decltype(t)::type, kMask>(images, mask_dev, n, h * w, channels_last != 0, pooled != 0, words, stream); });
}

}  // namespace focus
}  // namespace sx

extern "C" int sx_grey_statistics(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int pooled, long long* statistics_out, void* stream_ptr) {
    return sx::focus::grey_statistics_call<false>(images, dtype, n, h, w, channels_last, pooled, nullptr, statistics_out, stream_ptr);
}

extern "C" int sx_grey_statistics_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int pooled, const unsigned char* mask_dev,
                                         long long* statistics_out, void* stream_ptr) {
    return sx::focus::grey_statistics_call<true>(images, dtype, n, h, w, channels_last, pooled, mask_dev, statistics_out, stream_ptr);
}
