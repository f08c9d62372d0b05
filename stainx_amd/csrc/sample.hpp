// Tissue pixel sampling (included at the end of api.hip): a fixed-shape tile of at most K masked-in pixels per tile or per batch, chosen by
// an exact integer rule and copied bit for bit (sx_sample_pixels).  DESIGN.md 5j.
//
// The rule (include/stainx_hip.h states it in full): a group's masked-in pixels are ranked 0 .. n-1 in raster order (pooled: tile after
// tile).  n <= K: slot r holds rank r, the slots n .. K-1 are zero bytes with valid = 0.  n > K: slot j holds rank (j n + o) div K,
// o = offset mod n.
//
// Three launches, no memset, no workgroup waiting on another, nothing on the host:
//   count    one workgroup per chunk of kChunk mask bytes: the chunk's masked-in count, from 16-byte loads per lane.
//   scan     one workgroup per group: the exclusive prefix of the chunk counts (a chunk's first rank), n, taken = min(n, K), o, and -- the
//            rule turned round -- the first slot of every chunk: rank(j) >= R  <=>  j >= J(R) = max(0, ceil((R K - o) / n)), so the slots whose
//            rank lies in a chunk with first rank R0 and C masked-in pixels are exactly J(R0) .. J(R0 + C) - 1.  J(R0) of the next chunk is
//            J(R0 + C): the slot ranges of a group's chunks tile 0 .. taken-1, every slot has ONE writer.
//   scatter  the count launch's chunks again: a chunk without a slot leaves at once.  Otherwise the ranks inside the chunk are formed again
//            (a lane's 16 mask bits, wave64 ballots of the bits of its count with popcount prefixes, a per-wave offset in LDS), and a thread
//            per slot finds its rank's lane by bisection in LDS, the pixel in the lane's bits, and copies three values as integers of
//            the element's width.  The slots taken .. K-1 of a group are zeroed by the group's workgroups, strided.
//
// A chunk is a window of kChunk bytes of the mask at 16-byte ALIGNED addresses: a tile whose first mask byte sits `mis` bytes past an
// aligned address has its pixel p at window position p + mis, and a lane's 16 positions are one aligned 16-byte word.  A word that
// lies wholly inside the tile is one 16-byte load; the at most two words per tile that straddle its ends are read byte by byte, the
// bytes outside the tile never.  So any width and any mask pointer take the wide path.
#pragma once

#include "common.hpp"

namespace sx {
namespace sample {

constexpr int kChunk = 4096;                             // mask bytes per workgroup: 256 lanes x one 16-byte word
constexpr int kLaneBytes = 16;
constexpr int64_t kMaxSample = 1ll << 24;
static_assert(kChunk == kStreamThreads * kLaneBytes, "a chunk is one 16-byte word per lane");

static size_t align_up_256(size_t bytes) { return (bytes + 255) / 256 * 256; }
static int64_t chunks_per_tile(int64_t pixels) { return (pixels + (kLaneBytes - 1) + kChunk - 1) / kChunk; }      // (whatever the misalignment)

struct Layout {
    size_t offsets, slots, ranks, total;
};
static Layout layout(int64_t n_tiles, int64_t pixels) {
    const size_t chunks = (size_t)n_tiles * (size_t)chunks_per_tile(pixels);
    Layout l;
    l.offsets = 0;                                                                  // groups x uint64: o = offset mod n
    l.slots = align_up_256(sizeof(unsigned long long) * (size_t)n_tiles);           // chunks x uint32: count, then the chunk's first slot
    l.ranks = l.slots + align_up_256(sizeof(uint32_t) * chunks);                    // chunks x uint32: the chunk's first rank
    l.total = l.ranks + align_up_256(sizeof(uint32_t) * chunks);
    return l;
}

struct Args {
    const uint8_t* mask;               // (N, H*W) bytes, non-zero = in; null: every pixel
    unsigned long long* offsets;       // workspace
    uint32_t* slots;
    uint32_t* ranks;
    int32_t* taken;                    // outputs of the scan launch
    long long* population;
    uint8_t* valid;
    int64_t pixels, sample, offset;
    int blocks, pooled;                // chunks per tile
    int64_t n_tiles;
};

// Where the tile's first mask byte sits inside its aligned 16-byte word (0 without a mask).
__device__ __forceinline__ uint32_t misalignment(const Args& a, int64_t tile) {
    return a.mask ? (uint32_t)((reinterpret_cast<uintptr_t>(a.mask) + (uintptr_t)(tile * a.pixels)) & (uintptr_t)(kLaneBytes - 1)) : 0u;
}

// The four bytes of a word as four bits: byte i non-zero <=> bit i.
__device__ __forceinline__ uint32_t nonzero_nibble(uint32_t x) {
    const uint32_t high = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;      // bit 7 of every non-zero byte
    return (((high >> 7) * 0x01020408u) >> 24) & 0xfu;                                // b_i 2^(8i) -> b_i 2^(24+i); lower cross terms stay below bit 24
}

// The masked-in bits of a lane's 16 window positions v0 .. v0+15 (v0 a multiple of 16): bit i <=> pixel v0 + i - mis lies in the tile and
// its mask byte is non-zero.
template <bool kMask>
__device__ __forceinline__ uint32_t lane_bits(const uint8_t* __restrict__ tile_mask, uint32_t mis, int64_t pixels, int64_t v0) {
    const int64_t first = (int64_t)mis - v0, last = (int64_t)mis + pixels - v0;      // positions first .. last-1 of this word are pixels
    const int lo = (int)min(max(first, (int64_t)0), (int64_t)kLaneBytes), hi = (int)min(max(last, (int64_t)0), (int64_t)kLaneBytes);
    const uint32_t inside = (0xffffu >> (kLaneBytes - hi)) & (0xffffu << lo) & 0xffffu;      // bits lo .. hi-1; none where hi <= lo
    if (inside == 0u) return 0u;
    if constexpr (!kMask) return inside;
    const uint8_t* word = tile_mask + (v0 - (int64_t)mis);      // 16-byte aligned by construction
    if (inside == 0xffffu) {
        const uint4 q = *reinterpret_cast<const uint4*>(word);
        return nonzero_nibble(q.x) | (nonzero_nibble(q.y) << 4) | (nonzero_nibble(q.z) << 8) | (nonzero_nibble(q.w) << 12);
    }
    uint32_t bits = 0u;
    for (int i = lo; i < hi; ++i) bits |= (word[i] != 0 ? 1u : 0u) << i;
    return bits;
}

// A lane's count c (0 .. 16) -> the sum of the counts of the lanes below it in the wave, and the wave's sum: five ballots, one per bit of c.
__device__ __forceinline__ void wave_prefix(uint32_t c, uint32_t& below, uint32_t& total) {
    below = 0u;
    total = 0u;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const uint64_t m = __ballot((c >> b) & 1u);
        below += rank_in_mask(m) << b;
        total += (uint32_t)__popcll(m) << b;
    }
}

template <bool kMask>
__global__ __launch_bounds__(kStreamThreads) void sample_count_kernel(Args a) {
    __shared__ uint32_t wave_total[kStreamThreads / kWave];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk = (int)(blockIdx.x % (unsigned)a.blocks);
    const uint32_t mis = misalignment(a, tile);
    const uint32_t bits = lane_bits<kMask>(a.mask + tile * a.pixels, mis, a.pixels, (int64_t)chunk * kChunk + (int64_t)threadIdx.x * kLaneBytes);
    uint32_t below, total;
    wave_prefix((uint32_t)__popc(bits), below, total);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_total[threadIdx.x / kWave] = total;
    __syncthreads();
    if (threadIdx.x == 0) a.slots[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

// J(R): the first slot whose rank is at least R (n > K).
__device__ __forceinline__ uint32_t first_slot(unsigned long long rank, unsigned long long n, unsigned long long k, unsigned long long o) {
    const unsigned long long rk = rank * k;      // < 2^31 * 2^24
    return rk <= o ? 0u : (uint32_t)((rk - o + n - 1ull) / n);
}

// One workgroup per group.  A thread owns a run of consecutive chunks: it adds them up, the 256 sums are scanned in a fixed order (wave
// scans, the four wave sums through LDS), then it walks its run again and leaves every chunk's first rank and first slot.  Sums stay
// below 2^31: the entry point refuses larger groups.
__global__ __launch_bounds__(kStreamThreads) void sample_scan_kernel(Args a) {
    __shared__ uint32_t wave_total[kStreamThreads / kWave];
    const int64_t group = blockIdx.x;
    const int64_t chunks = a.pooled ? a.n_tiles * a.blocks : (int64_t)a.blocks;
    uint32_t* slots = a.slots + group * (int64_t)a.blocks;      // (pooled: group 0)
    uint32_t* ranks = a.ranks + group * (int64_t)a.blocks;
    const int64_t per = (chunks + kStreamThreads - 1) / kStreamThreads;
    const int64_t begin = min((int64_t)threadIdx.x * per, chunks), end = min(begin + per, chunks);
    uint32_t mine = 0u;
    for (int64_t i = begin; i < end; ++i) mine += slots[i];
    const uint32_t inclusive = wave_scan_u32(mine);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) wave_total[wave] = inclusive;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int q = 0; q < kStreamThreads / kWave; ++q) {
        if (q < wave) before += wave_total[q];
        total += wave_total[q];
    }
    const unsigned long long n = total, k = (unsigned long long)a.sample;
    const bool sub = n > k;
    const unsigned long long o = sub ? (unsigned long long)a.offset % n : 0ull;
    unsigned long long run = before + inclusive - mine;
    for (int64_t i = begin; i < end; ++i) {
        const uint32_t c = slots[i];
        ranks[i] = (uint32_t)run;
        slots[i] = sub ? first_slot(run, n, k, o) : (uint32_t)run;
        run += c;
    }
    if (threadIdx.x == 0) {
        a.offsets[group] = o;
        a.population[group] = (long long)n;
        a.taken[group] = (int32_t)(sub ? k : n);
    }
}

// E: an unsigned integer of the element's width -- a pixel's three values are moved, never converted.
template <typename E, bool kMask, bool kLast>
__global__ __launch_bounds__(kStreamThreads) void sample_scatter_kernel(const E* __restrict__ images, E* __restrict__ out, Args a) {
    __shared__ uint32_t lane_first[kStreamThreads];      // in-chunk rank of the lane's first masked-in pixel
    __shared__ uint32_t lane_mask[kStreamThreads];
    __shared__ uint32_t wave_total[kStreamThreads / kWave];
    const int64_t tile = blockIdx.x / (unsigned)a.blocks;
    const int chunk = (int)(blockIdx.x % (unsigned)a.blocks);
    const int64_t group = a.pooled ? 0 : tile;
    const int64_t group_chunks = a.pooled ? a.n_tiles * a.blocks : (int64_t)a.blocks;
    const int64_t in_group = a.pooled ? (int64_t)blockIdx.x : (int64_t)chunk;
    const int64_t k = a.sample;
    const int64_t taken = a.taken[group];
    E* dst = out + group * 3 * k;
    uint8_t* valid = a.valid + group * k;
    // the slots no pixel fills: zero bytes, valid = 0, shared out among the group's workgroups
    for (int64_t j = taken + in_group * kStreamThreads + threadIdx.x; j < k; j += group_chunks * kStreamThreads) {
        dst[j] = E(0);
        dst[k + j] = E(0);
        dst[2 * k + j] = E(0);
        valid[j] = 0;
    }
    const int64_t slot_begin = a.slots[blockIdx.x];
    const int64_t slot_end = in_group + 1 < group_chunks ? (int64_t)a.slots[blockIdx.x + 1] : taken;
    if (slot_begin >= slot_end) return;      // (uniform over the workgroup)
    const uint32_t mis = misalignment(a, tile);
    const int64_t v0 = (int64_t)chunk * kChunk + (int64_t)threadIdx.x * kLaneBytes;
    const uint32_t bits = lane_bits<kMask>(a.mask + tile * a.pixels, mis, a.pixels, v0);
    uint32_t below, total;
    wave_prefix((uint32_t)__popc(bits), below, total);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) wave_total[wave] = total;
    __syncthreads();
    uint32_t before = 0u;
    for (int q = 0; q < wave; ++q) before += wave_total[q];
    lane_first[threadIdx.x] = before + below;
    lane_mask[threadIdx.x] = bits;
    __syncthreads();
    const unsigned long long n = (unsigned long long)a.population[group], o = a.offsets[group];
    const unsigned long long first_rank = a.ranks[blockIdx.x];
    const bool sub = n > (unsigned long long)k;
    const E* img = images + tile * 3 * a.pixels;
    for (int64_t j = slot_begin + threadIdx.x; j < slot_end; j += kStreamThreads) {
        const unsigned long long rank = sub ? ((unsigned long long)j * n + o) / (unsigned long long)k : (unsigned long long)j;
        const uint32_t r = (uint32_t)(rank - first_rank);      // < the chunk's count
        int t = 0;                                             // the last lane whose first rank is <= r: it holds rank r
#pragma unroll
        for (int step = kStreamThreads / 2; step > 0; step >>= 1)
            if (lane_first[t + step] <= r) t += step;
        uint32_t m = lane_mask[t];
        for (uint32_t skip = r - lane_first[t]; skip > 0u; --skip) m &= m - 1u;
        const int64_t p = (int64_t)chunk * kChunk + (int64_t)t * kLaneBytes + (int64_t)(__ffs((int)m) - 1) - (int64_t)mis;
        E v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = kLast ? img[p * 3 + c] : img[c * a.pixels + p];
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c * k + j] = v[c];
        valid[j] = 1;
    }
}

template <typename E>
static void launch_all(const void* images, void* out, const Args& a, bool last, hipStream_t stream) {
    const unsigned grid = (unsigned)(a.n_tiles * a.blocks), groups = (unsigned)(a.pooled ? 1 : a.n_tiles);
    const E* img = static_cast<const E*>(images);
    E* dst = static_cast<E*>(out);
    if (a.mask)
        hipLaunchKernelGGL(sample_count_kernel<true>, dim3(grid), dim3(kStreamThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(sample_count_kernel<false>, dim3(grid), dim3(kStreamThreads), 0, stream, a);
    hipLaunchKernelGGL(sample_scan_kernel, dim3(groups), dim3(kStreamThreads), 0, stream, a);
    if (a.mask) {
        if (last) hipLaunchKernelGGL((sample_scatter_kernel<E, true, true>), dim3(grid), dim3(kStreamThreads), 0, stream, img, dst, a);
        else hipLaunchKernelGGL((sample_scatter_kernel<E, true, false>), dim3(grid), dim3(kStreamThreads), 0, stream, img, dst, a);
    } else {
        if (last) hipLaunchKernelGGL((sample_scatter_kernel<E, false, true>), dim3(grid), dim3(kStreamThreads), 0, stream, img, dst, a);
        else hipLaunchKernelGGL((sample_scatter_kernel<E, false, false>), dim3(grid), dim3(kStreamThreads), 0, stream, img, dst, a);
    }
}

static bool sizes_overflow(int64_t n, int64_t h, int64_t w) { return n > 0x7fffffffll || h > 0x7fffffffll || w > 0x7fffffffll || h * w >= (1ll << 31); }

}  // namespace sample
}  // namespace sx

extern "C" size_t sx_sample_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    using namespace sx::sample;
    if (n <= 0 || h <= 0 || w <= 0 || sizes_overflow(n, h, w)) return 0;
    if (chunks_per_tile(h * w) > 0x7fffffffll / n) return 0;
    return layout(n, h * w).total;
}

extern "C" int sx_sample_pixels(const void* images, int dtype, int64_t n, int64_t h, int64_t w, int channels_last, const uint8_t* mask_dev, int pooled, int64_t sample_size,
                                int64_t offset, void* pixels_out, uint8_t* valid_out, int32_t* taken_out, int64_t* population_out, void* ws, size_t ws_bytes, void* stream) {
    using namespace sx;
    using namespace sx::sample;
    const char* who = "sx_sample_pixels";
    if (!images) return fail(SX_ERR_BAD_ARG, "%s: images pointer is null", who);
    if (!pixels_out || !valid_out || !taken_out || !population_out) return fail(SX_ERR_BAD_ARG, "%s: an output pointer is null", who);
    if (dtype < SX_U8 || dtype > SX_F64) return fail(SX_ERR_DTYPE, "%s: unsupported dtype code %d", who, dtype);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SX_ERR_BAD_ARG, "%s: n, h, w must be positive, got n=%lld h=%lld w=%lld", who, (long long)n, (long long)h, (long long)w);
    if (sample_size < 1 || sample_size > kMaxSample) return fail(SX_ERR_BAD_ARG, "%s: sample_size must lie in 1 .. 2^24, got %lld", who, (long long)sample_size);
    if (offset < 0) return fail(SX_ERR_BAD_ARG, "%s: offset must not be negative, got %lld", who, (long long)offset);
    if (sizes_overflow(n, h, w) || (pooled && h * w > 0x7fffffffll / n))
        return fail(SX_ERR_BAD_ARG, "%s: a group must hold fewer than 2^31 pixels (n=%lld h=%lld w=%lld%s)", who, (long long)n, (long long)h, (long long)w, pooled ? ", pooled" : "");
    const int64_t pixels = h * w, blocks = chunks_per_tile(pixels);
    if (blocks > 0x7fffffffll / n) return fail(SX_ERR_BAD_ARG, "%s: n, h, w overflow one call: %lld work items", who, (long long)n * (long long)blocks);
    const Layout l = layout(n, pixels);
    if (!ws || ws_bytes < l.total) return fail(SX_ERR_BAD_ARG, "%s: workspace too small: need %zu bytes, got %zu", who, l.total, ws ? ws_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(ws) % 8 != 0) return fail(SX_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned", who);
    char* base = static_cast<char*>(ws);
    Args a;
    a.mask = mask_dev;
    a.offsets = reinterpret_cast<unsigned long long*>(base + l.offsets);
    a.slots = reinterpret_cast<uint32_t*>(base + l.slots);
    a.ranks = reinterpret_cast<uint32_t*>(base + l.ranks);
    a.taken = taken_out;
    a.population = reinterpret_cast<long long*>(population_out);
    a.valid = valid_out;
    a.pixels = pixels;
    a.sample = sample_size;
    a.offset = offset;
    a.blocks = (int)blocks;
    a.pooled = pooled != 0;
    a.n_tiles = n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool last = channels_last != 0;
    switch (dtype) {
        case SX_U8: launch_all<uint8_t>(images, pixels_out, a, last, s); break;
        case SX_F16:
        case SX_BF16: launch_all<uint16_t>(images, pixels_out, a, last, s); break;
        case SX_F32: launch_all<uint32_t>(images, pixels_out, a, last, s); break;
        default: launch_all<unsigned long long>(images, pixels_out, a, last, s); break;
    }
    return check_launch("pixel sampling");
}
