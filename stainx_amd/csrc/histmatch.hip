// Histogram matching for MI355X (gfx950): wavefront-private LDS histograms + fused LUT apply.
//
// Numerics follow HistogramMatchingTorch (rendeirolab/stainx src/stainx/backends/torch_backend.py:
// 134-301): pixels become uint8 grey levels (floats: trunc(clamp(x*255,0,255)), :115-120), one
// 256-bin histogram per channel pooled over the WHOLE batch (:229-236), source CDF vs reference CDF
// -> 256-entry float LUT with linear interpolation (:254-281), gather (:285), and the output range /
// dtype rules (:288-298).
//
// Kernels: (1) histogram -- 16-byte loads; planar layout: one plane chunk per workgroup and 32 bank-striped copies of
// the histogram in LDS (no bank conflicts); interleaved layout: one LDS sub-histogram per wave; integer adds only
// (bit-exact, order independent); (2) one small workgroup builds
// the 3 x 256 LUT (sequential double-precision prefix sums rounded to float per entry, exactly what
// torch.cumsum does on CPU floats) and the LUT in the OUTPUT element type; (3) apply -- LDS-resident
// typed LUT, 16-byte loads and stores, writes the final dtype directly (the reference's native path
// takes three more passes: histogram_matching.cu:153-166).
#include "common.hpp"
#include "dispatch.hpp"
#include "tissue.hpp"

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <type_traits>

namespace sx {
namespace histmatch {

constexpr int kBins = 256;
constexpr int kResSets = 16;            // one-launch form: sets of pooled counters per parity
constexpr int kResMaxChunks = 8192;     // ... and the most chunks (176 KB each) a batch may have to take it (1.4 GB)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

struct alignas(256) Tables {
    uint32_t counted[3][kBins];     // pooled integer histogram of the source batch as the last call counted it (for inspection)
    float lut[3][kBins];            // float LUT (torch_backend.py:276-281)
    uint64_t typed_lut[3][kBins];   // LUT already converted to the output element (low bytes)
    unsigned long long counts64[3][kBins];   // the histogram the LUT is built from (local, or all-reduced over ranks)
    // The live counters of the histogram pass.  Every entry point that counts also CONSUMES them (the kernel that reads them writes
    // zeros back), so a workspace that was zero before a call is zero after it: the *_ready entry points rely on that and skip the
    // hipMemsetAsync launch in front of the histogram pass (5 us of a 115 us call); the plain entry points clear them first.
    uint32_t counts[3][kBins];
    uint32_t status;                // bit 0: a *_ready call found counters that do not add up to the pixels it counted (workspace not ready)
#ifdef SX_DIAG
    // the one-launch form (histmatch_resident.hpp, diagnostic build): sets of pooled counters in two parities used alternately -- a call adds
    // into parity `res_parity` and clears the other -- and its chunk flags
    uint32_t res_counts[2][kResSets][3][kBins];
    uint32_t res_parity;
    uint32_t res_done, res_leave;         // chunks counted; workgroups that have left
    uint32_t res_flag[kResMaxChunks];     // chunk claimed for counting
    uint32_t res_flag2[kResMaxChunks];    // chunk claimed for the apply phase (or kept in somebody's registers)
    unsigned long long res_stamp[8];      // wall_clock64() of workgroup 0 at the phase boundaries of the one-launch form
#endif
};

struct Layout {
    int64_t n_tiles, pixels;        // pixels per tile (H*W)
    int channels_last;
    __device__ __forceinline__ int channel_of(int64_t e) const { return channels_last ? (int)(e % 3) : (int)((e / pixels) % 3); }
    __host__ __device__ int64_t elements() const { return n_tiles * 3 * pixels; }
};

template <typename T>
__device__ __forceinline__ uint32_t grey_level(T v) {
    if constexpr (sizeof(T) == 1) {
        return (uint32_t)v;
    } else {
        float x;
        if constexpr (sizeof(T) == 8) x = (float)v; else x = Elem<T>::load(v);
        return (uint32_t)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);     // torch_backend.py:119 (trunc)
    }
}

template <typename T> struct VecOf { static constexpr int n = 16 / sizeof(T); };   // elements per 16-byte load

// single elements (the calls that take packs count with histogram_planar_kernel / histogram_last_kernel)
template <typename T>
__global__ __launch_bounds__(kThreads) void histogram_kernel(const T* __restrict__ images, Layout lay, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[kWaves][3][kBins];
    for (int i = threadIdx.x; i < kWaves * 3 * kBins; i += kThreads) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t(*mine)[kBins] = hist[threadIdx.x / kWave];
    const int64_t total = lay.elements();
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) atomicAdd(&mine[lay.channel_of(e)][grey_level<T>(images[e])], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += (&hist[w][0][0])[i];
        if (s) atomicAdd(&counts[i], s);
    }
}

// Channels-last layout, 16-byte packs: the three channels alternate inside a pack, so three histograms are live: 16 copies of
// each (48 KB); word (channel*256 + bin)*16 + k lies in bank 16*(bin & 1) + k, so
// the four lanes that share a copy collide only when their bins have the same parity -- two lanes per bank on average where the
// per-wave histograms of histogram_kernel() put five.
constexpr int kLastCopies = 16;
constexpr int kLastChunk = 65536;       // elements (bytes for uint8) per workgroup; a multiple of 3 * V is not needed: the channel follows e % 3

// kPerTile: `total` is the elements of ONE tile (a multiple of V: a pack never straddles two tiles, and a tile starts on channel 0),
// workgroup b takes chunk b % chunks_per_tile of tile b / chunks_per_tile and adds into that tile's set of `counts` ([n][3][256]).
template <typename T, bool kPerTile = false>
__global__ __launch_bounds__(kThreads) void histogram_last_kernel(const T* __restrict__ images, int64_t total, uint32_t* __restrict__ counts, int chunks_per_tile = 1) {
    __shared__ uint32_t hist[3][kBins][kLastCopies];
    for (int i = threadIdx.x; i < 3 * kBins * kLastCopies; i += kThreads) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    constexpr int V = VecOf<T>::n;
    const int64_t tile = kPerTile ? blockIdx.x / chunks_per_tile : 0;
    if constexpr (kPerTile) {
        images += tile * total;
        counts += tile * 3 * kBins;
    }
    const int64_t begin = (int64_t)(kPerTile ? blockIdx.x % chunks_per_tile : blockIdx.x) * kLastChunk, end = min(begin + (int64_t)kLastChunk, total);
    const int copy = threadIdx.x & (kLastCopies - 1);
    for (int64_t e = begin + (int64_t)threadIdx.x * V; e < end; e += (int64_t)kThreads * V) {
        const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(images + e);
        int c = (int)(e % 3);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            atomicAdd(&hist[c][grey_level<T>(pk.v[i])][copy], 1u);
            c = c == 2 ? 0 : c + 1;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) {      // thread t adds up the copies of bin t of each channel, starting at its own bank
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kLastCopies; ++k) sum += (&hist[0][0][0])[i * kLastCopies + ((threadIdx.x + k) & (kLastCopies - 1))];
        if (sum) atomicAdd(&counts[i], sum);
    }
}

// torch.sum() of 256 contiguous float32 on the CPU (the reference's `counts.sum()` / `ref_hist.float().sum()`,
// torch_backend.py:141,222): not a plain running sum -- ATen's vectorised reduction keeps four accumulators of eight lanes
// over blocks of 32 elements, adds the accumulators in order, then the eight lanes in order.  Reproduced as is (verified
// against torch 2.10 on 300 random histograms, tools/check_torch_sum.py): a sum accumulated any other way differs in the
// last bit for ~20 % of histograms, which moves LUT entries by 1e-7 and flips a grey level at truncation boundaries.
template <class At>
__device__ inline float torch_sum_256(At at) {
    float acc[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[k][l] = 0.0f;
#pragma unroll 1      // (unrolled eight times it needs 140 registers: too many beside the histogram pass that also calls it)
    for (int i = 0; i < kBins / 32; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int l = 0; l < 8; ++l) acc[k][l] = __fadd_rn(acc[k][l], at(i * 32 + k * 8 + l));
    float total = 0.0f;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float lane = __fadd_rn(__fadd_rn(__fadd_rn(acc[0][l], acc[1][l]), acc[2][l]), acc[3][l]);
        total = l == 0 ? lane : __fadd_rn(total, lane);
    }
    return total;
}

// fit: normalised histogram  counts / (sum(counts) + 1e-8)  in float32 (torch_backend.py:139-141)
__global__ void normalise_kernel(Tables* __restrict__ tab, float* __restrict__ hist_out) {
    const int c = blockIdx.x;
    __shared__ float total_s;
    __shared__ float raw[kBins];
    const uint32_t count = tab->counts[c][threadIdx.x];
    tab->counts[c][threadIdx.x] = 0;      // consumed
    tab->counted[c][threadIdx.x] = count;
    raw[threadIdx.x] = (float)count;
    __syncthreads();
    if (threadIdx.x == 0) {
        total_s = torch_sum_256([&](int b) { return raw[b]; }) + 1e-8f;
    }
    __syncthreads();
    hist_out[c * kBins + threadIdx.x] = raw[threadIdx.x] / total_s;
}

template <typename O> __device__ __forceinline__ uint64_t pack_elem(O v) {
    uint64_t bits = 0;
    __builtin_memcpy(&bits, &v, sizeof(O));
    return bits;
}

__global__ void widen_kernel(Tables* __restrict__ tab, unsigned long long* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * kBins) {
        const uint32_t count = (&tab->counts[0][0])[i];
        (&tab->counts[0][0])[i] = 0;      // consumed
        (&tab->counted[0][0])[i] = count;
        out[i] = count;
    }
}

// One LUT entry: where the source's running sum s of grey level t falls among the reference's running sums.  InT decides the range
// rules of the output (:288-298).
__device__ __forceinline__ float lut_value(float s, const float* ref_cdf) {
    // searchsorted(right=False): first index with ref_cdf[idx] >= s; clamp to [1,255] (:260-261)
    int lo = 0, hi = kBins;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ref_cdf[mid] < s) lo = mid + 1; else hi = mid;
    }
    const int idx = min(max(lo, 1), kBins - 1);
    const float q_lo = ref_cdf[idx - 1], q_hi = ref_cdf[idx];
    const float diff = q_hi - q_lo;
    const float alpha = diff > 1e-10f ? (s - q_lo) / diff : 0.0f;                    // :272-273
    float v = (float)(idx - 1) + alpha * ((float)idx - (float)(idx - 1));             // :276
    if (s <= ref_cdf[0]) v = 0.0f;                                                    // :268, :279
    if (s >= ref_cdf[kBins - 1]) v = 255.0f;                                          // :269, :280
    return fminf(fmaxf(v, 0.0f), 255.0f);                                             // :281
}
// (the LUT value in the output element: what the apply pass stores)
template <typename T>
__device__ __forceinline__ T typed_value(float v) {
    if constexpr (sizeof(T) == 1) {
        return (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);                                // clamped like the float outputs, then truncated; a NaN is 0.
                                                                                      // (lut_value is inside 0..255 already; a GIVEN table -- sx_hm_apply_tables -- need not be, and the bare cast of 256, -1 or NaN is undefined)
    } else {
        const float unit = fminf(fmaxf(v / 255.0f, 0.0f), 1.0f);                      // :291, :296
        if constexpr (sizeof(T) == 8) return (double)unit; else return Elem<T>::store(unit);
    }
}
template <typename T>
__device__ __forceinline__ void lut_entry(Tables* __restrict__ tab, int c, int t, float s, const float* ref_cdf) {
    const float v = lut_value(s, ref_cdf);
    tab->lut[c][t] = v;
    tab->typed_lut[c][t] = pack_elem<T>(typed_value<T>(v));
}

// running sum in double rounded per entry (:236): the order is torch.cumsum's, so one thread per table walks it -- sixteen
// terms are fetched from LDS at a time (one LDS latency per term made the LUT kernel 11 us; the additions alone are ~1 us)
__device__ __forceinline__ void running_sum(const float* term, float* cdf) {
    double run = 0.0;
#pragma unroll 1
    for (int b0 = 0; b0 < kBins; b0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = term[b0 + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            run += (double)v[u];
            cdf[b0 + u] = (float)run;
        }
    }
}

// One workgroup of 256 threads per channel.
// (Round 4 tried the tables inside the APPLY launch -- every workgroup builds them from the final counters in its prologue, the workgroup
// that reads the counters last consumes them: same bits, 0.118 -> 0.142 ms per call.  Each workgroup runs six sequential chains of 256
// double-precision additions (torch.cumsum's order), and with eight workgroups per CU the chains of a CU share its four SIMDs: a 25 us
// prologue; with 1024-thread workgroups, two per CU, 0.124 ms -- still behind this 8.4 us launch of three workgroups.)
// (Tried: the LUT inside the histogram launch -- its first workgroup prepares the reference's running sums, the workgroup whose counts
// arrive last does the rest -- to save this launch and its boundary.  Same bits, and slower: 121 against 114 us per call.  Every one of
// the 3072 workgroups then waits for its counter adds to be acknowledged and for a ticket from ONE address before it may leave its
// CU: the histogram launch went from 36 to 57 us, more than this kernel's 8.8 us and the boundary together.)
// Per-tile form (sx_hm_transform_tiles): behind the Tables, one 3 x 256 set per tile of live counters, of the histogram as counted, of the
// float LUT and of the LUT in the output element (eight bytes reserved per entry, elements of T stored densely).  The live counters
// come first: one clear covers the pooled ones and them.
struct TileAreas {
    uint32_t* counts;       // [n][3][256] live, consumed by the LUT launch
    uint32_t* counted;      // [n][3][256]
    float* lut;             // [n][3][256]
    void* typed;            // [n][3][256] of the output element
    uint32_t* counts_out;   // the caller's copies (may be null)
    float* lut_out;
};
static size_t tile_area_bytes(int64_t n) { return (size_t)n * 3 * kBins * (3 * sizeof(uint32_t) + sizeof(uint64_t)); }
static TileAreas tile_areas(void* ws, int64_t n, uint32_t* counts_out, float* lut_out) {
    char* base = static_cast<char*>(ws) + sizeof(Tables);
    const size_t words = (size_t)n * 3 * kBins;
    return TileAreas{reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(base + 4 * words), reinterpret_cast<float*>(base + 8 * words), base + 12 * words, counts_out, lut_out};
}

// kPerTile: workgroup b serves channel b % 3 of tile b / 3 -- 3N independent chains, the reference's (which does not depend on the tile)
// beside each -- with the tile's own counters and tables; num_pixels is the pixels of ONE tile.
// kMasked (the tissue forms; always with a set per tile, one set for a pooled call): num_pixels is the TISSUE count -- the sum of the
// channel's own counters -- and the ready-state check compares that sum with the tissue pixels the histogram pass counted for the set
// (every channel with that one count: the three totals agree with each other and with the mask).
template <typename T, bool kPerTile, bool kMasked>
__device__ __forceinline__ void lut_body(Tables* __restrict__ tab, const unsigned long long* __restrict__ counts, const bool local, const float* __restrict__ ref_hist, double num_pixels, TileAreas tiles, const uint32_t* __restrict__ tissue_counts, unsigned long long* __restrict__ tissue_out) {
    const int c = kPerTile ? blockIdx.x % 3 : blockIdx.x, t = threadIdx.x;
    const size_t tile_entry = kPerTile ? ((size_t)blockIdx.x * kBins + t) : 0;      // (tile * 3 + c) * 256 + t
    __shared__ float src_cdf[kBins], ref_cdf[kBins];
    __shared__ float src_term[kBins], ref_term[kBins];
    __shared__ float ref_denom_s;
    __shared__ float ref_raw[kBins];
    // the divisions run one per thread; only the two running sums are sequential (that order is torch.cumsum's)
    ref_raw[t] = ref_hist[c * kBins + t];      // (one load per thread: the summing thread reading global memory itself paid eight round trips)
    __syncthreads();
    if (t == 64) {
        // reference: h / (sum(h) + 1e-8) (:222-223)
        ref_denom_s = torch_sum_256([&](int b) { return ref_raw[b]; }) + 1e-8f;
    }
    // source: counts / float(num_pixels + 1e-8) (:235)
    // (the local histogram is read as it was counted; counts pooled over ranks arrive widened to 64 bits)
    unsigned long long count;
    if (local) {
        uint32_t mine;
        if constexpr (kPerTile) {
            mine = tiles.counts[tile_entry];
            tiles.counts[tile_entry] = 0;
            tiles.counted[tile_entry] = mine;
            if (tiles.counts_out) tiles.counts_out[tile_entry] = mine;
        } else {
            mine = tab->counts[c][t];
            tab->counts[c][t] = 0;      // consumed: the next call's histogram pass starts from zero
            tab->counted[c][t] = mine;
        }
        count = mine;
        // the counters of a call add up to its pixels -- unless the workspace was not ready (see Tables)
        const double wave_total = wave_sum((double)mine);      // (integers below 2^53: exact)
        __shared__ double parts[kBins / kWave];
        if (lane_id() == 0) parts[t / kWave] = wave_total;
        __syncthreads();
        __shared__ double total_s;
        if (t == 0) {
            double total = 0.0;
            for (int w = 0; w < kBins / kWave; ++w) total += parts[w];
            if constexpr (kMasked) {
                const uint32_t set = blockIdx.x / 3;
                if (total != (double)tissue_counts[set]) atomicOr(&tab->status, 1u);
                if (c == 0 && tissue_out) tissue_out[set] = (unsigned long long)total;
                total_s = total;
            } else {
                if (total != num_pixels) atomicOr(&tab->status, 1u);
            }
        }
        if constexpr (kMasked) {
            __syncthreads();
            num_pixels = total_s;
        }
    } else {
        count = counts[c * kBins + t];
    }
    src_term[t] = (float)count / (float)(num_pixels + 1e-8);
    __syncthreads();
    ref_term[t] = ref_raw[t] / ref_denom_s;
    __syncthreads();
    if (t == 0) running_sum(src_term, src_cdf);
    else if (t == 64) running_sum(ref_term, ref_cdf);
    __syncthreads();
    if constexpr (kPerTile) {
        const float v = lut_value(src_cdf[t], ref_cdf);
        tiles.lut[tile_entry] = v;
        if (tiles.lut_out) tiles.lut_out[tile_entry] = v;
        static_cast<T*>(tiles.typed)[tile_entry] = typed_value<T>(v);
    } else {
        lut_entry<T>(tab, c, t, src_cdf[t], ref_cdf);
    }
}

template <typename T, bool kPerTile = false>
__global__ __launch_bounds__(kBins) void lut_kernel(Tables* __restrict__ tab, const unsigned long long* __restrict__ counts, const bool local, const float* __restrict__ ref_hist, double num_pixels, TileAreas tiles = TileAreas{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}) {
    lut_body<T, kPerTile, false>(tab, counts, local, ref_hist, num_pixels, tiles, nullptr, nullptr);
}
template <typename T>
__global__ __launch_bounds__(kBins) void lut_masked_kernel(Tables* __restrict__ tab, const float* __restrict__ ref_hist, TileAreas tiles, const uint32_t* __restrict__ tissue_counts, unsigned long long* __restrict__ tissue_out) {
    lut_body<T, true, true>(tab, nullptr, true, ref_hist, 0.0, tiles, tissue_counts, tissue_out);
}

// Planar layout, 16-byte packs: a workgroup takes one chunk of ONE channel plane, so a single 256-bin histogram is live
// and LDS has room for 32 copies of it, copy k in bank k: lane l only ever touches bank l % 32, so the 64 lanes of an
// atomic instruction never collide on a bank (random grey levels into a single histogram: ~5 of 64 lanes per bank and
// 13 cycles per instruction measured).  Integer adds: bit-exact.
// What bounds it (tools/histbench.hip, 201 MB of uint8, one MI355X): the LDS atomic unit takes one ds_add_u32 per ~6.7 cycles and
// CU whatever its lanes do (64, 32 or 16 active lanes and fixed conflict-free addresses: 39-40 us) -- 16 instructions per 16-byte
// pack, 38-39 us for the batch against 31 us for reading it.  Reaching that floor is a matter of waves per CU: 256 threads per
// 32 KB of copies left 46-49 us; 16 copies reach 39 us on noise and lose on slide background (four lanes of a wave on one
// address: 50 us); 512 threads SHARING the 32 copies, two packs in flight per thread: 38 us on noise, 36.5 us on background.
constexpr int kCopies = 32;
constexpr int kPlaneChunk = 65536;      // elements of one plane per workgroup
constexpr int kPlaneThreads = 512;
constexpr int kAhead = 2;               // packs loaded before the first of them is counted

// kPerTile: `counts` is [n][3][256] and plane p adds into the set of its tile p / 3.
template <typename T, bool kPerTile = false>
__global__ __launch_bounds__(kPlaneThreads) void histogram_planar_kernel(const T* __restrict__ images, Layout lay, int chunks_per_plane, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[kBins][kCopies];
    for (int i = threadIdx.x; i < kBins * kCopies; i += kPlaneThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    constexpr int V = VecOf<T>::n;
    const int64_t plane = blockIdx.x / chunks_per_plane, chunk = blockIdx.x % chunks_per_plane;
    const int channel = (int)(plane % 3);
    const T* src = images + plane * lay.pixels;
    const int64_t begin = chunk * (int64_t)kPlaneChunk, end = min(begin + (int64_t)kPlaneChunk, lay.pixels);
    uint32_t* mine = &hist[0][threadIdx.x & (kCopies - 1)];
    constexpr int64_t kStride = (int64_t)kPlaneThreads * V;
    for (int64_t e = begin + (int64_t)threadIdx.x * V; e < end; e += kStride * kAhead) {
        Pack<T, V> pk[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a)
            if (e + a * kStride < end) pk[a] = *reinterpret_cast<const Pack<T, V>*>(src + e + a * kStride);
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            if (e + a * kStride < end) {
#pragma unroll
                for (int i = 0; i < V; ++i) atomicAdd(&mine[grey_level<T>(pk[a].v[i]) * kCopies], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kBins) {   // thread t adds up the copies of bin t, starting at its own bank
        const int t = threadIdx.x;
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kCopies; ++k) sum += hist[t][(t + k) & (kCopies - 1)];
        if (sum) atomicAdd(&counts[(kPerTile ? (plane / 3) * 3 * kBins : 0) + channel * kBins + t], sum);
    }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(kThreads) void apply_kernel(const T* __restrict__ images, T* __restrict__ out, Layout lay, const Tables* __restrict__ tab) {
    __shared__ T lut[3][kBins];
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) {
        const uint64_t bits = (&tab->typed_lut[0][0])[i];
        T v;
        __builtin_memcpy(&v, &bits, sizeof(T));
        (&lut[0][0])[i] = v;
    }
    __syncthreads();
    const int64_t total = lay.elements();
    constexpr int V = kVec ? VecOf<T>::n : 1;
    const int64_t stride = (int64_t)gridDim.x * kThreads * V;
    for (int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V; e0 < total; e0 += stride) {
        // Back to front: the histogram pass read the batch front to back, so this pass starts on what the Infinity Cache got last (config 3,
        // rotating two batches, A/B on one box: 0.1213 / 0.1201 -> 0.1188 / 0.1179 ms per call).
        const int64_t e = total - V - e0;
        if constexpr (kVec) {
            const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(images + e);      // (non-temporal loads here: no gain over rotating batches, 3 us lost on one buffer -- tools/ab_rotating_siblings.py)
            Pack<T, V> res;
            int c = lay.channel_of(e);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                res.v[i] = lut[c][grey_level<T>(pk.v[i])];
                if (lay.channels_last) c = c == 2 ? 0 : c + 1;
            }
            store_pack_stream<T, V>(out + e, res.v);      // non-temporal: written once, not read again by this library
        } else {
            out[e] = lut[lay.channel_of(e)][grey_level<T>(images[e])];
        }
    }
}

// ---- per-tile form: the fallback histogram (single elements: odd sizes, unaligned views) and the apply pass ----------------------------
// workgroup b counts share b % blocks_per_tile of tile b / blocks_per_tile, one LDS sub-histogram per wave as histogram_kernel()
template <typename T>
__global__ __launch_bounds__(kThreads) void histogram_tile_kernel(const T* __restrict__ images, Layout lay, int blocks_per_tile, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[kWaves][3][kBins];
    for (int i = threadIdx.x; i < kWaves * 3 * kBins; i += kThreads) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t(*mine)[kBins] = hist[threadIdx.x / kWave];
    const int64_t tile = blockIdx.x / blocks_per_tile, per_tile = 3 * lay.pixels;
    const T* src = images + tile * per_tile;
    for (int64_t e = (int64_t)(blockIdx.x % blocks_per_tile) * kThreads + threadIdx.x; e < per_tile; e += (int64_t)blocks_per_tile * kThreads)
        atomicAdd(&mine[lay.channel_of(e)][grey_level<T>(src[e])], 1u);      // (e inside the tile: a tile starts on channel 0 in both layouts)
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += (&hist[w][0][0])[i];
        if (s) atomicAdd(&counts[tile * 3 * kBins + i], s);
    }
}

// A workgroup applies ONE tile's LUT (from the tile's typed table into LDS) to one chunk of that tile.  Back to front like apply_kernel():
// workgroup 0 takes the last chunk of the last tile, and a chunk is walked from its end.
constexpr int kTilePacks = 16;      // packs (or single elements) per thread and chunk
template <typename T, bool kVec>
__global__ __launch_bounds__(kThreads) void apply_tiles_kernel(const T* __restrict__ images, T* __restrict__ out, Layout lay, int chunks_per_tile, const T* __restrict__ typed) {
    constexpr int V = kVec ? VecOf<T>::n : 1;
    constexpr int64_t kChunk = (int64_t)kThreads * V * kTilePacks;
    const int64_t work = (int64_t)gridDim.x - 1 - blockIdx.x;
    const int64_t tile = work / chunks_per_tile, chunk = work % chunks_per_tile, per_tile = 3 * lay.pixels;
    __shared__ T lut[3][kBins];
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) (&lut[0][0])[i] = typed[tile * 3 * kBins + i];
    __syncthreads();
    const T* src = images + tile * per_tile;
    T* dst = out + tile * per_tile;
    const int64_t begin = chunk * kChunk, end = min(begin + kChunk, per_tile);      // (vector path: per_tile % V == 0, so is end - begin)
    for (int64_t e0 = (int64_t)threadIdx.x * V; e0 < end - begin; e0 += (int64_t)kThreads * V) {
        const int64_t e = end - V - e0;
        if constexpr (kVec) {
            const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(src + e);
            Pack<T, V> res;
            int c = lay.channel_of(e);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                res.v[i] = lut[c][grey_level<T>(pk.v[i])];
                if (lay.channels_last) c = c == 2 ? 0 : c + 1;
            }
            store_pack_stream<T, V>(dst + e, res.v);
        } else {
            dst[e] = lut[lay.channel_of(e)][grey_level<T>(src[e])];
        }
    }
}

// ---- tissue masks: pixel-wise kernels ---------------------------------------------------------------------------------------------------
// The rule needs a pixel's three channels, and the planar kernels above see one channel plane per workgroup.  The masked forms are
// therefore PIXEL-WISE in both layouts: a thread holds one 16-byte pack of each of the three planes (planar) or three consecutive packs
// (interleaved) -- VP = 16 / sizeof(T) whole pixels --, decides each pixel once (the caller's mask bytes, or the rule of tissue.hpp on the
// pixel's linear-light values: a 256-entry table for uint8) and counts / replaces the three elements of a tissue pixel.  Three
// histograms are live: 16 bank-striped copies of each (48 KB, the layout of histogram_last_kernel).  No mask is written or read in
// the rule form: each pass reads the pixels and nothing else.  (DESIGN.md 5c weighs this against a mask written first.)
constexpr int kMaskTrips = 8;      // packs per thread and work item

// (the layout is a template argument: with a run-time branch between the two pack forms the compiler keeps the pixels in scratch memory)
template <typename T, int VP, bool kLast>
__device__ __forceinline__ void load_pixels(const T* __restrict__ tile, int64_t pixels, int64_t p, T (&v)[3][VP]) {
    if constexpr (VP == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][0] = tile[kLast ? p * 3 + c : c * pixels + p];
    } else if constexpr (kLast) {
        const Pack<T, VP> first = *reinterpret_cast<const Pack<T, VP>*>(tile + 3 * p), second = *reinterpret_cast<const Pack<T, VP>*>(tile + 3 * p + VP),
                          third = *reinterpret_cast<const Pack<T, VP>*>(tile + 3 * p + 2 * VP);
#pragma unroll
        for (int k = 0; k < 3 * VP; ++k) v[k % 3][k / 3] = k < VP ? first.v[k % VP] : k < 2 * VP ? second.v[k % VP] : third.v[k % VP];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Pack<T, VP> pk = *reinterpret_cast<const Pack<T, VP>*>(tile + c * pixels + p);
#pragma unroll
            for (int i = 0; i < VP; ++i) v[c][i] = pk.v[i];
        }
    }
}
template <typename T, int VP, bool kLast>
__device__ __forceinline__ void store_pixels(T* __restrict__ tile, int64_t pixels, int64_t p, const T (&v)[3][VP]) {
    if constexpr (VP == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) tile[kLast ? p * 3 + c : c * pixels + p] = v[c][0];
    } else if constexpr (kLast) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            T piece[VP];
#pragma unroll
            for (int i = 0; i < VP; ++i) piece[i] = v[(j * VP + i) % 3][(j * VP + i) / 3];
            store_pack_stream<T, VP>(tile + 3 * p + j * VP, piece);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) store_pack_stream<T, VP>(tile + c * pixels + p, v[c]);
    }
}
// bit i: pixel i of the pack is tissue (uniform branch: a call has a mask or it has none)
template <typename T, int VP>
__device__ __forceinline__ uint32_t pixel_bits(const tissue::Source& tis, int64_t pixel_index, const T (&v)[3][VP], const LinearTable& table) {
    uint32_t in = 0u;
    if (tis.mask) {
        if constexpr (VP == 1) {
            in = tis.mask[pixel_index] ? 1u : 0u;
        } else {
            const Pack<uint8_t, VP> m = *reinterpret_cast<const Pack<uint8_t, VP>*>(tis.mask + pixel_index);
#pragma unroll
            for (int i = 0; i < VP; ++i) in |= m.v[i] ? (1u << i) : 0u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < VP; ++i)
            in |= tissue::is_tissue(tissue::linear_of<T>(v[0][i], table), tissue::linear_of<T>(v[1][i], table), tissue::linear_of<T>(v[2][i], table), tis.y_cut) ? (1u << i) : 0u;
    }
    return in;
}

// workgroup b: work item b % chunks_per_tile of tile b / chunks_per_tile; its counts go to set `tile` (per_tile) or set 0 of `counts`
// ([sets][3][256]), its tissue pixels to the set's word of `tissue_counts`
template <typename T, bool kVec, bool kLast>
__global__ __launch_bounds__(kThreads) void histogram_masked_kernel(const T* __restrict__ images, Layout lay, int chunks_per_tile, int per_tile, tissue::Source tis, uint32_t* __restrict__ counts, uint32_t* __restrict__ tissue_counts) {
    constexpr int VP = kVec ? VecOf<T>::n : 1;
    __shared__ uint32_t hist[3][kBins][kLastCopies];
    __shared__ LinearTable table;
    for (int i = threadIdx.x; i < 3 * kBins * kLastCopies; i += kThreads) (&hist[0][0][0])[i] = 0;
    if constexpr (sizeof(T) == 1) table.fill();
    __syncthreads();
    const int64_t tile = blockIdx.x / chunks_per_tile;
    const int64_t set = per_tile ? tile : 0;
    const T* src = images + tile * 3 * lay.pixels;
    const int64_t begin = (int64_t)(blockIdx.x % chunks_per_tile) * kThreads * VP * kMaskTrips, end = min(begin + (int64_t)kThreads * VP * kMaskTrips, lay.pixels);
    const int copy = threadIdx.x & (kLastCopies - 1);
    uint32_t mine = 0;
    for (int64_t p = begin + (int64_t)threadIdx.x * VP; p < end; p += (int64_t)kThreads * VP) {
        T v[3][VP];
        load_pixels<T, VP, kLast>(src, lay.pixels, p, v);
        const uint32_t in = pixel_bits<T, VP>(tis, tile * lay.pixels + p, v, table);
        mine += (uint32_t)__builtin_popcount(in);
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            if ((in >> i) & 1u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) atomicAdd(&hist[c][grey_level<T>(v[c][i])][copy], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) {      // thread t adds up the copies of bin t of each channel, starting at its own bank
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kLastCopies; ++k) sum += (&hist[0][0][0])[i * kLastCopies + ((threadIdx.x + k) & (kLastCopies - 1))];
        if (sum) atomicAdd(&counts[set * 3 * kBins + i], sum);
    }
    const uint32_t wave_tissue = wave_total_u32(mine);
    if (lane_id() == 0 && wave_tissue) atomicAdd(&tissue_counts[set], wave_tissue);
}

// a tissue pixel gets its LUT values, a background pixel the bits of its input elements (floats are not quantised)
template <typename T, bool kVec, bool kLast>
__global__ __launch_bounds__(kThreads) void apply_masked_kernel(const T* __restrict__ images, T* __restrict__ out, Layout lay, int chunks_per_tile, int per_tile, tissue::Source tis, const T* __restrict__ typed) {
    constexpr int VP = kVec ? VecOf<T>::n : 1;
    // (uint8: a fourth row, the identity, and the row chosen by arithmetic on the pixel's bit -- sixteen pixels' selects on compare masks
    // do not fit the scalar registers)
    __shared__ T lut[sizeof(T) == 1 ? 4 : 3][kBins];
    __shared__ LinearTable table;
    const int64_t tile = blockIdx.x / chunks_per_tile;
    const int64_t set = per_tile ? tile : 0;
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) (&lut[0][0])[i] = typed[set * 3 * kBins + i];
    if constexpr (sizeof(T) == 1) {
        for (int i = threadIdx.x; i < kBins; i += kThreads) lut[3][i] = (T)i;
        table.fill();
    }
    __syncthreads();
    const T* src = images + tile * 3 * lay.pixels;
    T* dst = out + tile * 3 * lay.pixels;
    const int64_t begin = (int64_t)(blockIdx.x % chunks_per_tile) * kThreads * VP * kMaskTrips, end = min(begin + (int64_t)kThreads * VP * kMaskTrips, lay.pixels);
    for (int64_t p = begin + (int64_t)threadIdx.x * VP; p < end; p += (int64_t)kThreads * VP) {
        T v[3][VP];
        load_pixels<T, VP, kLast>(src, lay.pixels, p, v);
        const uint32_t in = pixel_bits<T, VP>(tis, tile * lay.pixels + p, v, table);
#pragma unroll
        for (int i = 0; i < VP; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (sizeof(T) == 1) v[c][i] = lut[3 - (int)((in >> i) & 1u) * (3 - c)][grey_level<T>(v[c][i])];
                else v[c][i] = (in >> i) & 1u ? lut[c][grey_level<T>(v[c][i])] : v[c][i];
            }
        store_pixels<T, VP, kLast>(dst, lay.pixels, p, v);
    }
}

// fit: the pooled tissue histogram of set 0, normalised as normalise_kernel() does
__global__ void normalise_masked_kernel(Tables* __restrict__ tab, uint32_t* __restrict__ counts, uint32_t* __restrict__ counted, const uint32_t* __restrict__ tissue_counts, float* __restrict__ hist_out, unsigned long long* __restrict__ tissue_out) {
    const int c = blockIdx.x, t = threadIdx.x;
    __shared__ float total_s;
    __shared__ float raw[kBins];
    __shared__ double parts[kBins / kWave];
    const uint32_t count = counts[c * kBins + t];
    counts[c * kBins + t] = 0;      // consumed
    counted[c * kBins + t] = count;
    raw[t] = (float)count;
    const double wave_total = wave_sum((double)count);
    if (lane_id() == 0) parts[t / kWave] = wave_total;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int w = 0; w < kBins / kWave; ++w) total += parts[w];
        if (total != (double)tissue_counts[0]) atomicOr(&tab->status, 1u);
        if (c == 0 && tissue_out) tissue_out[0] = (unsigned long long)total;
        total_s = torch_sum_256([&](int b) { return raw[b]; }) + 1e-8f;
    }
    __syncthreads();
    hist_out[c * kBins + t] = raw[t] / total_s;
}

// ---- slide level: the histogram pass as a call of its own, tables from GIVEN counts, the apply pass with GIVEN tables ----
// The export step of sx_hm_estimate(_masked), behind the histogram kernels above: workgroup b widens channel b % 3 of set b / 3 to 64
// bits, consumes the live counters and runs the ready-state check of lut_body() -- the set's counters add up to `expected` pixels
// (kMasked: to the tissue pixels the histogram pass counted for the set).  pixels_out: that total (may be null).
template <bool kMasked>
__global__ __launch_bounds__(kBins) void export_counts_kernel(Tables* __restrict__ tab, uint32_t* __restrict__ live, uint32_t* __restrict__ counted, unsigned long long* __restrict__ counts_out,
                                                              unsigned long long* __restrict__ pixels_out, double expected, const uint32_t* __restrict__ tissue_counts) {
    const int c = blockIdx.x % 3, t = threadIdx.x;
    const uint32_t set = blockIdx.x / 3;
    const size_t entry = (size_t)blockIdx.x * kBins + t;      // (set * 3 + c) * 256 + t
    __shared__ double parts[kBins / kWave];
    const uint32_t mine = live[entry];
    live[entry] = 0;      // consumed
    counted[entry] = mine;
    counts_out[entry] = mine;
    const double wave_total = wave_sum((double)mine);      // (integers below 2^53: exact)
    if (lane_id() == 0) parts[t / kWave] = wave_total;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int w = 0; w < kBins / kWave; ++w) total += parts[w];
        if (total != (kMasked ? (double)tissue_counts[set] : expected)) atomicOr(&tab->status, 1u);
        if (c == 0 && pixels_out) pixels_out[set] = (unsigned long long)total;
    }
}

// sx_hm_tables: lut_body()'s arithmetic on GIVEN 64-bit counts and pixel totals (device memory), workgroup b: channel b % 3 of set b / 3.
// A set without pixels gets the identity table: the reference's arithmetic would give 0 / 1e-8 = 0 in every bin, a running sum of
// zeros and so a table of zeros -- black; it never sees such a source, and a slide without tissue is better left as it is.
__global__ __launch_bounds__(kBins) void tables_kernel(const unsigned long long* __restrict__ counts, const unsigned long long* __restrict__ pixels, const float* __restrict__ ref_hist, float* __restrict__ lut_out) {
    const int c = blockIdx.x % 3, t = threadIdx.x;
    const size_t entry = (size_t)blockIdx.x * kBins + t;
    const unsigned long long n_pixels = pixels[blockIdx.x / 3];
    if (n_pixels == 0) {      // (uniform in the workgroup)
        lut_out[entry] = (float)t;
        return;
    }
    __shared__ float src_cdf[kBins], ref_cdf[kBins];
    __shared__ float src_term[kBins], ref_term[kBins];
    __shared__ float ref_denom_s;
    __shared__ float ref_raw[kBins];
    ref_raw[t] = ref_hist[c * kBins + t];
    __syncthreads();
    if (t == 64) ref_denom_s = torch_sum_256([&](int b) { return ref_raw[b]; }) + 1e-8f;      // :222-223
    src_term[t] = (float)counts[entry] / (float)((double)n_pixels + 1e-8);                      // :235
    __syncthreads();
    ref_term[t] = ref_raw[t] / ref_denom_s;
    __syncthreads();
    if (t == 0) running_sum(src_term, src_cdf);
    else if (t == 64) running_sum(ref_term, ref_cdf);
    __syncthreads();
    lut_out[entry] = lut_value(src_cdf[t], ref_cdf);
}

// sx_hm_apply_tables: apply_tiles_kernel() with GIVEN float tables.  A workgroup converts its source's 768 floats to the output element
// in its prologue (table `tile` of `lut`, or table 0 for every tile when there is one source); no typed table in a workspace.
template <typename T, bool kVec, bool kLast>
__global__ __launch_bounds__(kThreads) void apply_tables_kernel(const T* __restrict__ images, T* __restrict__ out, int64_t pixels, int chunks_per_tile, const float* __restrict__ tables, int per_tile) {
    constexpr int V = kVec ? VecOf<T>::n : 1;
    constexpr int64_t kChunk = (int64_t)kThreads * V * kTilePacks;
    const int64_t work = (int64_t)gridDim.x - 1 - blockIdx.x;
    const int64_t tile = work / chunks_per_tile, chunk = work % chunks_per_tile, per_tile_elems = 3 * pixels;
    __shared__ T lut[3][kBins];
    const float* mine = tables + (per_tile ? tile * 3 * kBins : 0);
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) (&lut[0][0])[i] = typed_value<T>(mine[i]);
    __syncthreads();
    const T* src = images + tile * per_tile_elems;
    T* dst = out + tile * per_tile_elems;
    const int64_t begin = chunk * kChunk, end = min(begin + kChunk, per_tile_elems);      // (vector path: per_tile_elems % V == 0, so is end - begin)
    for (int64_t e0 = (int64_t)threadIdx.x * V; e0 < end - begin; e0 += (int64_t)kThreads * V) {
        const int64_t e = end - V - e0;
        int c = kLast ? (int)(e % 3) : (int)(e >= pixels) + (int)(e >= 2 * pixels);      // (planar: a pack never straddles planes)
        if constexpr (kVec) {
            const Pack<T, V> pk = *reinterpret_cast<const Pack<T, V>*>(src + e);
            Pack<T, V> res;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                res.v[i] = lut[c][grey_level<T>(pk.v[i])];
                if constexpr (kLast) c = c == 2 ? 0 : c + 1;
            }
            store_pack_stream<T, V>(dst + e, res.v);
        } else {
            dst[e] = lut[c][grey_level<T>(src[e])];
        }
    }
}

// sx_hm_apply_tables_masked: apply_masked_kernel() with GIVEN float tables, converted in the prologue as above
template <typename T, bool kVec, bool kLast>
__global__ __launch_bounds__(kThreads) void apply_tables_masked_kernel(const T* __restrict__ images, T* __restrict__ out, Layout lay, int chunks_per_tile, int per_tile, tissue::Source tis, const float* __restrict__ tables) {
    constexpr int VP = kVec ? VecOf<T>::n : 1;
    __shared__ T lut[sizeof(T) == 1 ? 4 : 3][kBins];      // (uint8: the fourth row is the identity, see apply_masked_kernel)
    __shared__ LinearTable table;
    const int64_t tile = blockIdx.x / chunks_per_tile;
    const float* mine = tables + (per_tile ? tile * 3 * kBins : 0);
    for (int i = threadIdx.x; i < 3 * kBins; i += kThreads) (&lut[0][0])[i] = typed_value<T>(mine[i]);
    if constexpr (sizeof(T) == 1) {
        for (int i = threadIdx.x; i < kBins; i += kThreads) lut[3][i] = (T)i;
        table.fill();
    }
    __syncthreads();
    const T* src = images + tile * 3 * lay.pixels;
    T* dst = out + tile * 3 * lay.pixels;
    const int64_t begin = (int64_t)(blockIdx.x % chunks_per_tile) * kThreads * VP * kMaskTrips, end = min(begin + (int64_t)kThreads * VP * kMaskTrips, lay.pixels);
    for (int64_t p = begin + (int64_t)threadIdx.x * VP; p < end; p += (int64_t)kThreads * VP) {
        T v[3][VP];
        load_pixels<T, VP, kLast>(src, lay.pixels, p, v);
        const uint32_t in = pixel_bits<T, VP>(tis, tile * lay.pixels + p, v, table);
#pragma unroll
        for (int i = 0; i < VP; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (sizeof(T) == 1) v[c][i] = lut[3 - (int)((in >> i) & 1u) * (3 - c)][grey_level<T>(v[c][i])];
                else v[c][i] = (in >> i) & 1u ? lut[c][grey_level<T>(v[c][i])] : v[c][i];
            }
        store_pixels<T, VP, kLast>(dst, lay.pixels, p, v);
    }
}

#ifdef SX_DIAG
}  // namespace histmatch
}  // namespace sx
#include "histmatch_resident.hpp"
namespace sx {
namespace histmatch {
#endif

static size_t workspace_bytes() { return sizeof(Tables); }

#ifdef SX_DIAG
// The one-launch form (histmatch_resident.hpp): planar uint8 batches of at least 32 MB whose planes are whole sweeps.  One workgroup per CU
// (an ordinary launch: the kernel does not depend on its workgroups being resident together).
static int device_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = -1;
        cached[dev] = n;
    }
    return cached[dev] > 0 ? cached[dev] : 0;
}
static bool resident_shape(int64_t n, int64_t pixels) {
    const int64_t sweeps = pixels % kResSweepBytes == 0 ? n * 3 * (pixels / kResSweepBytes) : 0;
    return sweeps >= 2048 && (sweeps + kResChunkSweeps - 1) / kResChunkSweeps <= kResMaxChunks;      // (at least 32 MB: smaller batches are bound by latency either way)
}
static bool run_resident(const uint8_t* images, uint8_t* out, int64_t n, int64_t pixels, Tables* tab, const float* ref_hist, hipStream_t stream) {
    const int cus = device_cus();
    if (cus <= 0) return false;
    const int64_t total_sweeps = n * 3 * (pixels / kResSweepBytes);
    const int sweeps_per_plane = (int)(pixels / kResSweepBytes);
    const int64_t chunks = (total_sweeps + kResChunkSweeps - 1) / kResChunkSweeps;
    const unsigned grid = (unsigned)std::min<int64_t>(cus, chunks);
    hipLaunchKernelGGL(resident_kernel, dim3(grid), dim3(kResThreads), 0, stream, images, out, total_sweeps, sweeps_per_plane, tab, ref_hist, (double)(n * pixels));
    return true;
}
#endif

// The per-tile calls (and sx_hm_estimate, pooled or not): the per-tile areas behind the Tables.  The masked calls: behind the Tables one
// tissue counter per set, then the per-tile areas of `sets` sets (a pooled call: one set).  One clear covers the pooled live counters, the
// status word, (masked) the tissue counters and the sets' live counters: any contents in, READY out.
static size_t tiles_workspace_bytes(int64_t n) { return workspace_bytes() + tile_area_bytes(n); }
static size_t masked_tissue_bytes(int64_t n) { return (sizeof(uint32_t) * (size_t)n + 255) / 256 * 256; }
static size_t masked_workspace_bytes(int64_t n) { return workspace_bytes() + masked_tissue_bytes(n) + tile_area_bytes(n); }
static int clear_counters(Tables* tab, size_t behind_tables, hipStream_t stream) {
    if (hipMemsetAsync(tab->counts, 0, sizeof(Tables) - offsetof(Tables, counts) + behind_tables, stream) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    return SX_OK;
}

// 16-byte packs: the images and (where there is one) the output at 16-byte aligned addresses, and whole packs in what a pack must not
// leave -- a channel plane of a planar tile; of channels-last tiles the batch, or the tile where the call keeps tiles apart
// (within_tile); with a mask the pixels of a tile in both layouts, and a pack's mask bytes aligned.  Single elements otherwise.
template <typename T>
static bool vector_path(const Layout& lay, const void* images, const void* out, bool within_tile, bool masked = false, const uint8_t* mask = nullptr) {
    constexpr int V = VecOf<T>::n;
    const auto aligned = [](const void* p, size_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; };      // (a null pointer: no such operand)
    const int64_t whole = (masked || !lay.channels_last) ? lay.pixels : (within_tile ? 3 * lay.pixels : lay.elements());
    return aligned(images, 16) && aligned(out, 16) && whole % V == 0 && aligned(mask, V);
}

// The histogram pass of the unmasked calls: planar packs, channels-last packs or single elements, into the pooled counters or (kPerTile)
// the tiles' own.
template <typename T, bool kPerTile>
static void histogram_pass(const T* in, const Layout& lay, bool vec, uint32_t* counts, hipStream_t stream) {
    const int64_t n = lay.n_tiles, per_tile = 3 * lay.pixels, total = lay.elements();
    if (vec && !lay.channels_last) {
        const int chunks_per_plane = (int)((lay.pixels + kPlaneChunk - 1) / kPlaneChunk);
        hipLaunchKernelGGL((histogram_planar_kernel<T, kPerTile>), dim3((unsigned)(n * 3 * chunks_per_plane)), dim3(kPlaneThreads), 0, stream, in, lay, chunks_per_plane, counts);
    } else if (vec) {
        const int chunks_per_tile = kPerTile ? (int)((per_tile + kLastChunk - 1) / kLastChunk) : 1;
        const unsigned grid = kPerTile ? (unsigned)(n * chunks_per_tile) : (unsigned)((total + kLastChunk - 1) / kLastChunk);
        hipLaunchKernelGGL((histogram_last_kernel<T, kPerTile>), dim3(grid), dim3(kThreads), 0, stream, in, kPerTile ? per_tile : total, counts, chunks_per_tile);
    } else if constexpr (kPerTile) {
        const int blocks_per_tile = (int)std::min<int64_t>((per_tile + kThreads * 4 - 1) / (kThreads * 4), 64);
        hipLaunchKernelGGL((histogram_tile_kernel<T>), dim3((unsigned)(n * blocks_per_tile)), dim3(kThreads), 0, stream, in, lay, blocks_per_tile, counts);
    } else {
        const unsigned grid = (unsigned)std::min<int64_t>((total + kThreads * 4 - 1) / (kThreads * 4), 256 * 8);
        hipLaunchKernelGGL((histogram_kernel<T>), dim3(grid), dim3(kThreads), 0, stream, in, lay, counts);
    }
}

template <typename T>
static int run(const void* images, void* out, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, float* hist_out, unsigned long long* counts_out, const unsigned long long* counts_in, double n_total, void* ws, hipStream_t stream, bool ready) {
    const Layout lay{n, h * w, channels_last};
    Tables* tab = static_cast<Tables*>(ws);
    const T* in = static_cast<const T*>(images);
    const bool vec = vector_path<T>(lay, images, out, /*within_tile=*/false);
    const int64_t per_block = (int64_t)kThreads * (vec ? VecOf<T>::n : 1) * 4;
    const unsigned grid = (unsigned)std::min<int64_t>((lay.elements() + per_block - 1) / per_block, 256 * 8);
    double lut_pixels = n_total;
    if (!counts_in) {
        if (!ready) {
            if (const int rc = clear_counters(tab, 0, stream)) return rc;
        }
#ifdef SX_DIAG
        if constexpr (std::is_same<T, uint8_t>::value) {
            static const int mode = [] { const char* e = std::getenv("SX_HM_RESIDENT"); return e ? std::atoi(e) : 1; }();
            if (mode != 0 && vec && !channels_last && out && !hist_out && !counts_out && resident_shape(n, lay.pixels)) {
                if (run_resident(in, static_cast<uint8_t*>(out), n, lay.pixels, tab, ref_hist, stream)) return check_launch("histogram transform (one launch)");
            }
        }
#endif
        histogram_pass<T, false>(in, lay, vec, &tab->counts[0][0], stream);
        if (hist_out) {
            hipLaunchKernelGGL(normalise_kernel, dim3(3), dim3(kBins), 0, stream, tab, hist_out);
            return check_launch("histogram fit");
        }
        if (counts_out) {
            hipLaunchKernelGGL(widen_kernel, dim3(3), dim3(kBins), 0, stream, tab, counts_out);
            return check_launch("histogram counts");
        }
        lut_pixels = (double)(n * h * w);
    }
    hipLaunchKernelGGL((lut_kernel<T>), dim3(3), dim3(kBins), 0, stream, tab, counts_in, counts_in == nullptr, ref_hist, lut_pixels);
    if (vec)
        hipLaunchKernelGGL((apply_kernel<T, true>), dim3(grid), dim3(kThreads), 0, stream, in, static_cast<T*>(out), lay, tab);
    else
        hipLaunchKernelGGL((apply_kernel<T, false>), dim3(grid), dim3(kThreads), 0, stream, in, static_cast<T*>(out), lay, tab);
    return check_launch("histogram transform");
}

// One histogram and one LUT per tile: clear, histogram pass, 3N LUT workgroups, apply pass
template <typename T>
static int run_tiles(const void* images, void* out, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, uint32_t* counts_out, float* lut_out, void* ws, hipStream_t stream) {
    const Layout lay{n, h * w, channels_last};
    Tables* tab = static_cast<Tables*>(ws);
    const TileAreas areas = tile_areas(ws, n, counts_out, lut_out);
    const T* in = static_cast<const T*>(images);
    const bool vec = vector_path<T>(lay, images, out, /*within_tile=*/true);
    if (const int rc = clear_counters(tab, sizeof(uint32_t) * (size_t)n * 3 * kBins, stream)) return rc;
    histogram_pass<T, true>(in, lay, vec, areas.counts, stream);
    hipLaunchKernelGGL((lut_kernel<T, true>), dim3((unsigned)(3 * n)), dim3(kBins), 0, stream, tab, nullptr, true, ref_hist, (double)lay.pixels, areas);
    const int64_t chunk = (int64_t)kThreads * (vec ? VecOf<T>::n : 1) * kTilePacks;
    const int chunks_per_tile = (int)((3 * lay.pixels + chunk - 1) / chunk);
    if (vec)
        hipLaunchKernelGGL((apply_tiles_kernel<T, true>), dim3((unsigned)(n * chunks_per_tile)), dim3(kThreads), 0, stream, in, static_cast<T*>(out), lay, chunks_per_tile, static_cast<const T*>(areas.typed));
    else
        hipLaunchKernelGGL((apply_tiles_kernel<T, false>), dim3((unsigned)(n * chunks_per_tile)), dim3(kThreads), 0, stream, in, static_cast<T*>(out), lay, chunks_per_tile, static_cast<const T*>(areas.typed));
    return check_launch("histogram transform (per tile)");
}

// The masked calls: the histogram pass over tissue, then the normalised histogram (hist_out), the counts alone (counts64_out:
// sx_hm_estimate_masked) or the tables and the apply pass.
template <typename T>
static int run_masked(const void* images, void* out, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, float* hist_out, tissue::Source tis, bool per_tile, uint32_t* counts_out, float* lut_out, unsigned long long* tissue_out, void* ws, hipStream_t stream, unsigned long long* counts64_out) {
    const Layout lay{n, h * w, channels_last};
    Tables* tab = static_cast<Tables*>(ws);
    const int64_t sets = per_tile ? n : 1;
    uint32_t* tissue_counts = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + sizeof(Tables));
    const TileAreas areas = tile_areas(static_cast<char*>(ws) + masked_tissue_bytes(n), sets, counts_out, lut_out);
    const T* in = static_cast<const T*>(images);
    const bool vec = vector_path<T>(lay, images, out, /*within_tile=*/true, /*masked=*/true, tis.mask);
    if (const int rc = clear_counters(tab, masked_tissue_bytes(n) + sizeof(uint32_t) * (size_t)sets * 3 * kBins, stream)) return rc;
    const int64_t chunk = (int64_t)kThreads * (vec ? VecOf<T>::n : 1) * kMaskTrips;
    const int chunks_per_tile = (int)((lay.pixels + chunk - 1) / chunk);
    const dim3 grid((unsigned)(n * chunks_per_tile)), block(kThreads);
    with_flags(vec, channels_last != 0, [&](auto kVec, auto kLast) {
        hipLaunchKernelGGL((histogram_masked_kernel<T, decltype(kVec)::value, decltype(kLast)::value>), grid, block, 0, stream, in, lay, chunks_per_tile, per_tile ? 1 : 0, tis, areas.counts, tissue_counts);
    });
    if (hist_out) {
        hipLaunchKernelGGL(normalise_masked_kernel, dim3(3), dim3(kBins), 0, stream, tab, areas.counts, areas.counted, tissue_counts, hist_out, tissue_out);
        return check_launch("histogram fit (tissue mask)");
    }
    if (counts64_out) {
        hipLaunchKernelGGL((export_counts_kernel<true>), dim3((unsigned)(3 * sets)), dim3(kBins), 0, stream, tab, areas.counts, areas.counted, counts64_out, tissue_out, 0.0, tissue_counts);
        return check_launch("histogram estimate (tissue mask)");
    }
    hipLaunchKernelGGL((lut_masked_kernel<T>), dim3((unsigned)(3 * sets)), dim3(kBins), 0, stream, tab, ref_hist, areas, tissue_counts, tissue_out);
    with_flags(vec, channels_last != 0, [&](auto kVec, auto kLast) {
        hipLaunchKernelGGL((apply_masked_kernel<T, decltype(kVec)::value, decltype(kLast)::value>), grid, block, 0, stream, in, static_cast<T*>(out), lay, chunks_per_tile, per_tile ? 1 : 0, tis, static_cast<const T*>(areas.typed));
    });
    return check_launch("histogram transform (tissue mask)");
}

static int check_tile_count(int64_t n) {      // (3 n workgroups of the table launches, 64 work items per tile of the histogram pass)
    if (n * 3 > 0x7fffffffll / 64) return fail(SX_ERR_BAD_ARG, "too many tiles for one call: %lld", (long long)n);
    return SX_OK;
}

// what sx_hm_transform_tiles and sx_hm_estimate check behind their pointers: both run on the per-tile workspace
static int check_tiles_call(int dtype, int64_t n, int64_t h, int64_t w, const void* ws, size_t ws_bytes) {
    if (const int rc = check_sizes_got(n, h, w)) return rc;
    if (const int rc = check_tile_count(n)) return rc;
    if (const int rc = dtype_ok(dtype)) return rc;
    return check_workspace(ws, ws_bytes, tiles_workspace_bytes(n));
}

static int dispatch_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, float* hist_out, const uint8_t* mask, double threshold, int per_tile, uint32_t* counts_out, float* lut_out, unsigned long long* tissue_out, void* ws, size_t ws_bytes, void* stream_ptr, unsigned long long* counts64_out = nullptr) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (const int rc = check_sizes_got(n, h, w)) return rc;
    if (const int rc = check_tile_count(n)) return rc;
    if (const int rc = tissue::check_source(mask, threshold)) return rc;
    if (const int rc = dtype_ok(dtype)) return rc;
    if (const int rc = check_workspace(ws, ws_bytes, masked_workspace_bytes(n))) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const tissue::Source tis = tissue::source_of(mask, threshold);
    return with_dtype(dtype, [&](auto t) { return run_masked<typename decltype(t)::type>(images, out, n, h, w, channels_last, ref_hist, hist_out, tis, per_tile != 0, counts_out, lut_out, tissue_out, ws, stream, counts64_out); });
}

static int dispatch(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, float* hist_out, unsigned long long* counts_out, const unsigned long long* counts_in, double n_total, void* ws, size_t ws_bytes, void* stream_ptr, bool ready = false) {
    if (!images) return fail(SX_ERR_BAD_ARG, "images pointer is null");
    if (const int rc = check_sizes_got(n, h, w)) return rc;
    if (const int rc = check_workspace(ws, ws_bytes, workspace_bytes())) return rc;      // (the dtype code: with_dtype, below)
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return run<typename decltype(t)::type>(images, out, n, h, w, channels_last, ref_hist, hist_out, counts_out, counts_in, n_total, ws, stream, ready); });
}

// sx_hm_estimate: one clear, the histogram pass of run_tiles() (per tile) or run() (pooled), the export launch.  The workspace has the
// per-tile layout either way; a pooled call counts into the Tables' own live counters.
template <typename T>
static int run_estimate(const void* images, int64_t n, int64_t h, int64_t w, int channels_last, bool per_tile, unsigned long long* counts_out, unsigned long long* pixels_out, void* ws, hipStream_t stream) {
    const Layout lay{n, h * w, channels_last};
    Tables* tab = static_cast<Tables*>(ws);
    const TileAreas areas = tile_areas(ws, n, nullptr, nullptr);
    const T* in = static_cast<const T*>(images);
    const bool vec = vector_path<T>(lay, images, nullptr, per_tile);
    if (const int rc = clear_counters(tab, per_tile ? sizeof(uint32_t) * (size_t)n * 3 * kBins : 0, stream)) return rc;
    if (per_tile) {
        histogram_pass<T, true>(in, lay, vec, areas.counts, stream);
        hipLaunchKernelGGL((export_counts_kernel<false>), dim3((unsigned)(3 * n)), dim3(kBins), 0, stream, tab, areas.counts, areas.counted, counts_out, pixels_out, (double)lay.pixels, nullptr);
    } else {
        histogram_pass<T, false>(in, lay, vec, &tab->counts[0][0], stream);
        hipLaunchKernelGGL((export_counts_kernel<false>), dim3(3), dim3(kBins), 0, stream, tab, &tab->counts[0][0], &tab->counted[0][0], counts_out, pixels_out, (double)(n * lay.pixels), nullptr);
    }
    return check_launch("histogram estimate");
}

// sx_hm_apply_tables(_masked): ONE launch, the float tables read by the kernel; the pack rule and the work items of run_masked() (masked)
// or run_tiles()
template <typename T>
static int run_apply_tables(const void* images, void* out, int64_t n, int64_t h, int64_t w, int channels_last, const float* tables, int64_t n_sources, tissue::Source tis, bool masked, hipStream_t stream) {
    const Layout lay{n, h * w, channels_last};
    const T* in = static_cast<const T*>(images);
    T* dst = static_cast<T*>(out);
    const int per_tile = n_sources > 1 ? 1 : 0;      // (n_sources == n_tiles == 1: table 0 either way)
    const bool vec = vector_path<T>(lay, images, out, /*within_tile=*/true, masked, tis.mask);
    const int64_t chunk = (int64_t)kThreads * (vec ? VecOf<T>::n : 1) * (masked ? kMaskTrips : kTilePacks);
    const int64_t chunks_per_tile = ((masked ? lay.pixels : 3 * lay.pixels) + chunk - 1) / chunk;
    if (n * chunks_per_tile > 0x7fffffffll) return fail(SX_ERR_BAD_ARG, "batch too large for one launch: %lld tiles of %lld pixels", (long long)n, (long long)lay.pixels);
    const dim3 grid((unsigned)(n * chunks_per_tile)), block(kThreads);
    with_flags(vec, channels_last != 0, [&](auto kVec, auto kLast) {
        if (masked) hipLaunchKernelGGL((apply_tables_masked_kernel<T, decltype(kVec)::value, decltype(kLast)::value>), grid, block, 0, stream, in, dst, lay, (int)chunks_per_tile, per_tile, tis, tables);
        else hipLaunchKernelGGL((apply_tables_kernel<T, decltype(kVec)::value, decltype(kLast)::value>), grid, block, 0, stream, in, dst, lay.pixels, (int)chunks_per_tile, tables, per_tile);
    });
    return check_launch(masked ? "histogram apply with given tables (tissue mask)" : "histogram apply with given tables");
}

static int dispatch_apply_tables(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* tables, int64_t n_sources, bool masked, const uint8_t* mask, double threshold, void* stream_ptr) {
    if (!images || !out || !tables) return fail(SX_ERR_BAD_ARG, "images / out / lut pointer is null");
    if (const int rc = check_sizes_got(n, h, w)) return rc;
    if (n_sources != 1 && n_sources != n) return fail(SX_ERR_BAD_ARG, "n_sources must be 1 or n_tiles = %lld, got %lld", (long long)n, (long long)n_sources);
    if (masked) {
        if (const int rc = tissue::check_source(mask, threshold)) return rc;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    const tissue::Source tis = masked ? tissue::source_of(mask, threshold) : tissue::Source{mask, 0.0f};
    return with_dtype(dtype, [&](auto t) { return run_apply_tables<typename decltype(t)::type>(images, out, n, h, w, channels_last, tables, n_sources, tis, masked, stream); });
}

}  // namespace histmatch
}  // namespace sx

using namespace sx;

extern "C" size_t sx_hm_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return histmatch::workspace_bytes();
}

extern "C" int sx_hm_fit(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, float* hist_out, void* ws, size_t ws_bytes, void* stream) {
    if (!hist_out) return fail(SX_ERR_BAD_ARG, "hist_out pointer is null");
    return histmatch::dispatch(images, nullptr, dtype, n, h, w, channels_last, nullptr, hist_out, nullptr, nullptr, 0.0, ws, ws_bytes, stream);
}

extern "C" int sx_hm_transform(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_hist) return fail(SX_ERR_BAD_ARG, "out / ref_hist pointer is null");
    return histmatch::dispatch(images, out, dtype, n, h, w, channels_last, ref_hist, nullptr, nullptr, nullptr, 0.0, ws, ws_bytes, stream);
}

// The same calls on a workspace in the READY state -- zero-filled by sx_hm_workspace_init() or left behind by any completed call of
// this section on it: no clearing launch in front of the histogram pass.  A workspace that was not ready is noticed (the counters do
// not add up to the pixels counted) and reported by sx_hm_workspace_status(); the result of that call is not to be used.
extern "C" int sx_hm_workspace_init(void* ws, size_t ws_bytes, void* stream) {
    if (!ws || ws_bytes < histmatch::workspace_bytes()) return fail(SX_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", histmatch::workspace_bytes(), ws_bytes);
    if (hipMemsetAsync(ws, 0, histmatch::workspace_bytes(), static_cast<hipStream_t>(stream)) != hipSuccess) return fail(SX_ERR_LAUNCH, "hipMemsetAsync failed");
    return SX_OK;
}

extern "C" size_t sx_hm_workspace_status_offset(void) { return offsetof(histmatch::Tables, status); }
#ifdef SX_DIAG
// (tests and tools: the word every call in the one-launch form toggles; its phase stamps)
extern "C" size_t sx_hm_workspace_parity_offset(void) { return offsetof(histmatch::Tables, res_parity); }
extern "C" size_t sx_debug_hm_stamp_offset(void) { return offsetof(histmatch::Tables, res_stamp); }
#endif

extern "C" int sx_hm_fit_ready(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, float* hist_out, void* ws, size_t ws_bytes, void* stream) {
    if (!hist_out) return fail(SX_ERR_BAD_ARG, "hist_out pointer is null");
    return histmatch::dispatch(images, nullptr, dtype, n, h, w, channels_last, nullptr, hist_out, nullptr, nullptr, 0.0, ws, ws_bytes, stream, true);
}

extern "C" int sx_hm_transform_ready(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_hist) return fail(SX_ERR_BAD_ARG, "out / ref_hist pointer is null");
    return histmatch::dispatch(images, out, dtype, n, h, w, channels_last, ref_hist, nullptr, nullptr, nullptr, 0.0, ws, ws_bytes, stream, true);
}

extern "C" int sx_hm_counts_ready(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, unsigned long long* counts_out, void* ws, size_t ws_bytes, void* stream) {
    if (!counts_out) return fail(SX_ERR_BAD_ARG, "counts_out pointer is null");
    return histmatch::dispatch(images, nullptr, dtype, n, h, w, channels_last, nullptr, nullptr, counts_out, nullptr, 0.0, ws, ws_bytes, stream, true);
}

// Source histogram pooled ACROSS RANKS: local integer counts out (3 x 256 u64), all-reduce on the host side, apply with the global counts.
extern "C" int sx_hm_counts(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, unsigned long long* counts_out, void* ws, size_t ws_bytes, void* stream) {
    if (!counts_out) return fail(SX_ERR_BAD_ARG, "counts_out pointer is null");
    return histmatch::dispatch(images, nullptr, dtype, n, h, w, channels_last, nullptr, nullptr, counts_out, nullptr, 0.0, ws, ws_bytes, stream);
}

extern "C" int sx_hm_apply(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const unsigned long long* counts, double n_total_pixels, const float* ref_hist, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !counts || !ref_hist) return fail(SX_ERR_BAD_ARG, "out / counts / ref_hist pointer is null");
    if (!(n_total_pixels >= 1.0)) return fail(SX_ERR_BAD_ARG, "n_total_pixels must be >= 1");
    return histmatch::dispatch(images, out, dtype, n, h, w, channels_last, ref_hist, nullptr, nullptr, counts, n_total_pixels, ws, ws_bytes, stream);
}

// One histogram and one LUT per TILE against the one reference (scikit-image's match_histograms, tiatoolbox and HistomicsTK work on ONE
// image): the pooled kernels with a set of counters and tables per tile behind the pooled Tables.
extern "C" size_t sx_hm_tiles_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return histmatch::tiles_workspace_bytes(n);
}

extern "C" int sx_hm_transform_tiles(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, uint32_t* tile_counts_out, float* tile_lut_out, void* ws, size_t ws_bytes, void* stream_ptr) {
    if (!images || !out || !ref_hist) return fail(SX_ERR_BAD_ARG, "images / out / ref_hist pointer is null");
    if (const int rc = histmatch::check_tiles_call(dtype, n, h, w, ws, ws_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return histmatch::run_tiles<typename decltype(t)::type>(images, out, n, h, w, channels_last, ref_hist, tile_counts_out, tile_lut_out, ws, stream); });
}

// ---- tissue masks: histograms over tissue pixels only, background pixels copied (an extension) --------------------------------------------
extern "C" size_t sx_hm_masked_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return histmatch::masked_workspace_bytes(n);
}

extern "C" int sx_hm_fit_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const uint8_t* mask, double luminosity_threshold, float* hist_out, unsigned long long* tissue_count_out, void* ws, size_t ws_bytes, void* stream) {
    if (!hist_out) return fail(SX_ERR_BAD_ARG, "hist_out pointer is null");
    return histmatch::dispatch_masked(images, nullptr, dtype, n, h, w, channels_last, nullptr, hist_out, mask, luminosity_threshold, 0, nullptr, nullptr, tissue_count_out, ws, ws_bytes, stream);
}

extern "C" int sx_hm_transform_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* ref_hist, const uint8_t* mask, double luminosity_threshold, int per_tile, uint32_t* counts_out, float* lut_out, unsigned long long* tissue_counts_out, void* ws, size_t ws_bytes, void* stream) {
    if (!out || !ref_hist) return fail(SX_ERR_BAD_ARG, "out / ref_hist pointer is null");
    return histmatch::dispatch_masked(images, out, dtype, n, h, w, channels_last, ref_hist, nullptr, mask, luminosity_threshold, per_tile, counts_out, lut_out, tissue_counts_out, ws, ws_bytes, stream);
}

// ---- slide level: estimate histograms, build tables from given counts, apply given tables (an extension) --------------------
extern "C" int sx_hm_estimate(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int per_tile, unsigned long long* counts_out, unsigned long long* pixels_out, void* ws, size_t ws_bytes, void* stream_ptr) {
    if (!images || !counts_out) return fail(SX_ERR_BAD_ARG, "images / counts_out pointer is null");
    if (const int rc = histmatch::check_tiles_call(dtype, n, h, w, ws, ws_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_ptr);
    return with_dtype(dtype, [&](auto t) { return histmatch::run_estimate<typename decltype(t)::type>(images, n, h, w, channels_last, per_tile != 0, counts_out, pixels_out, ws, stream); });
}

extern "C" int sx_hm_estimate_masked(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, int per_tile, const uint8_t* mask, double luminosity_threshold, unsigned long long* counts_out, unsigned long long* pixels_out, void* ws, size_t ws_bytes, void* stream) {
    if (!counts_out) return fail(SX_ERR_BAD_ARG, "counts_out pointer is null");
    return histmatch::dispatch_masked(images, nullptr, dtype, n, h, w, channels_last, nullptr, nullptr, mask, luminosity_threshold, per_tile, nullptr, nullptr, pixels_out, ws, ws_bytes, stream, counts_out);
}

extern "C" int sx_hm_tables(const unsigned long long* counts, const unsigned long long* pixels, int64_t n_sets, const float* ref_hist, float* lut_out, void* stream) {
    if (!counts || !pixels || !ref_hist || !lut_out) return fail(SX_ERR_BAD_ARG, "counts / pixels / ref_hist / lut_out pointer is null");
    if (n_sets <= 0 || n_sets * 3 > 0x7fffffffll / 64) return fail(SX_ERR_BAD_ARG, "n_sets must be positive and at most %lld, got %lld", 0x7fffffffll / 64 / 3, (long long)n_sets);
    hipLaunchKernelGGL(histmatch::tables_kernel, dim3((unsigned)(3 * n_sets)), dim3(histmatch::kBins), 0, static_cast<hipStream_t>(stream), counts, pixels, ref_hist, lut_out);
    return check_launch("histogram tables");
}

extern "C" int sx_hm_apply_tables(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* lut, int64_t n_sources, void* stream) {
    return histmatch::dispatch_apply_tables(images, out, dtype, n, h, w, channels_last, lut, n_sources, false, nullptr, 0.0, stream);
}

extern "C" int sx_hm_apply_tables_masked(const void* images, void* out, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const float* lut, int64_t n_sources, const uint8_t* mask, double luminosity_threshold, void* stream) {
    return histmatch::dispatch_apply_tables(images, out, dtype, n, h, w, channels_last, lut, n_sources, true, mask, luminosity_threshold, stream);
}
