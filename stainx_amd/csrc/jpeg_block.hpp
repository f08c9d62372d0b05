// The block arithmetic and the index arithmetic of the JPEG round trip (jpeg.hpp: sx_jpeg_roundtrip): baseline JPEG's lossy part as
// libjpeg implements it, in int32, with no HIP dependency -- tools/jpeg_block_check.cpp compiles this file for the host alone and runs it
// under the sanitizers.  The rule is stated in include/stainx_hip.h and DESIGN.md 4w; what is here is what the kernel calls.
//   D(x, n) = (x + (1 << (n - 1))) >> n, >> arithmetic.  Multiplications by 4 / 8192 stand where libjpeg shifts left: the operand may be
//   negative.
#ifndef SX_JPEG_BLOCK_HPP
#define SX_JPEG_BLOCK_HPP

#include <cmath>
#include <cstdint>

#ifndef __HIPCC__      // (tools/jpeg_block_check.cpp compiles the arithmetic for the host alone)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define SX_JPEG_FN __host__ __device__ __attribute__((always_inline)) inline      // (a block lives in registers: every index must fold to a constant)
#define SX_JPEG_MEMBER __host__ __device__ __attribute__((always_inline))          // (a call that is not inlined puts its reference arguments in scratch)

namespace sx {
namespace jpeg_block {

constexpr int kJpegRegionW = 128;          // a workgroup's region: 128 columns by
constexpr int kJpegRegionH444 = 64;        //   64 rows in 4:4:4 (three full planes on chip),
constexpr int kJpegRegionH420 = 128;       //   128 rows in 4:2:0 (one full plane and two quarter planes with their halo)
constexpr int kJpegPitch = 144;            // bytes of a row of a full-resolution plane on chip (128 + 16: block rows two apart start 32 banks apart)
constexpr int kJpegHalo = 8;               // 4:2:0: chroma samples decoded beyond the region on each side (one block; the filter reads one sample)
constexpr int kJpegChromaSide = kJpegRegionW / 2 + 2 * kJpegHalo;      // 80: rows and columns of the chroma window of a 128 x 128 region
constexpr int kJpegChromaPitch = kJpegChromaSide;
constexpr int kJpegPlaneBytes444 = kJpegRegionH444 * kJpegPitch;
constexpr int kJpegLumaBytes420 = kJpegRegionH420 * kJpegPitch;
constexpr int kJpegChromaBytes420 = kJpegChromaSide * kJpegChromaPitch;
constexpr int kJpegBytes444 = 3 * kJpegPlaneBytes444, kJpegBytes420 = kJpegLumaBytes420 + 2 * kJpegChromaBytes420;
constexpr int kJpegPlaneBytes = kJpegBytes444 > kJpegBytes420 ? kJpegBytes444 : kJpegBytes420;      // 31 232
static_assert(kJpegRegionH420 == kJpegRegionW && kJpegRegionW % 16 == 0 && kJpegRegionH444 % 16 == 0, "regions are aligned to 16 pixels; the chroma window is square");
static_assert(kJpegPitch % 8 == 0 && kJpegChromaPitch % 8 == 0 && kJpegLumaBytes420 % 8 == 0 && kJpegChromaBytes420 % 8 == 0 && kJpegPlaneBytes444 % 8 == 0, "a block's row is an aligned 8-byte word");

SX_JPEG_FN int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
SX_JPEG_FN int jpeg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the quality and the tables -----------------------------------------------------------------------------------------------------
// The quality of a tile: 0 = leave the tile (NaN, infinite, < 1), else min((int)q, 100).
SX_JPEG_FN int jpeg_quality(float q) {
    if (!(q >= 1.0f) || q == __builtin_huge_valf()) return 0;      // (false for a NaN; +inf -- every finite quality from 100 up, FLT_MAX included, is 100)
    return q >= 100.0f ? 100 : (int)q;
}
// Annex K's tables in natural (row-major) order; `chroma`: the chrominance table.
SX_JPEG_FN int jpeg_base(int chroma, int i) {
    const unsigned char luminance[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                         18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    const unsigned char chrominance[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    return chroma ? chrominance[i] : luminance[i];
}
// Q[i] of a quality 1..100.
SX_JPEG_FN int jpeg_table_entry(int quality, int chroma, int i) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    return jpeg_clamp((jpeg_base(chroma, i) * scale + 50) / 100, 1, 255);
}
// The quantiser divides by 8 Q (8 .. 2040).  M = ceil(2^32 / d) makes floor(n / d) the high word of n M for every n with n d < 2^32
// (the error M d - 2^32 is below d, so n (M d - 2^32) < 2^32 leaves the quotient's floor alone): here n < 2^18 and d < 2^11.
SX_JPEG_FN uint32_t jpeg_magic(int q_entry) { return 0xFFFFFFFFu / (uint32_t)(8 * q_entry) + 1u; }
SX_JPEG_FN int jpeg_divide(uint32_t n, uint32_t magic) { return (int)(uint32_t)(((uint64_t)n * magic) >> 32); }
// Quantise and dequantise one coefficient (it carries the forward transform's factor of 8):  sign(c) ((|c| + (8 Q >> 1)) / (8 Q)) Q.
SX_JPEG_FN int jpeg_requantise(int c, int q_entry, uint32_t magic) {
    const int k = jpeg_divide((uint32_t)((c < 0 ? -c : c) + 4 * q_entry), magic) * q_entry;
    return c < 0 ? -k : k;
}

// ---- levels and colour ----------------------------------------------------------------------------------------------------------------
// The level of a float element (already float32): clamp(rint(255 x), 0, 255); a NaN is level 0.
SX_JPEG_FN int jpeg_level(float x) {
    const float v = rintf(x * 255.0f);
    return !(v >= 0.0f) ? 0 : (v > 255.0f ? 255 : (int)v);
}
SX_JPEG_FN int jpeg_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
SX_JPEG_FN int jpeg_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16; }
SX_JPEG_FN int jpeg_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16; }
SX_JPEG_FN void jpeg_to_rgb(int y, int cb, int cr, int (&rgb)[3]) {      // cb, cr as stored (0..255)
    cb -= 128;
    cr -= 128;
    rgb[0] = jpeg_clamp(y + ((91881 * cr + 32768) >> 16), 0, 255);
    rgb[1] = jpeg_clamp(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
    rgb[2] = jpeg_clamp(y + ((116130 * cb + 32768) >> 16), 0, 255);
}

// ---- the two transforms (jfdctint / jidctint: CONST_BITS 13, PASS1_BITS 2) ---------------------------------------------------------------
// The odd part both share: from (t4, t5, t6, t7) the four sums o[0..3]; forward: outputs 7, 5, 3, 1 before the descale.
SX_JPEG_FN void jpeg_odd_part(int t4, int t5, int t6, int t7, int (&o)[4]) {
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[0] = t4 + z1 + z3;
    o[1] = t5 + z2 + z4;
    o[2] = t6 + z2 + z3;
    o[3] = t7 + z1 + z4;
}
// One forward pass over eight values `stride` apart.
template <bool kRowPass>
SX_JPEG_FN void jpeg_forward_pass(int* d, int stride) {
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride], d7 = d[7 * stride];
    const int t0 = d0 + d7, t1 = d1 + d6, t2 = d2 + d5, t3 = d3 + d4, t7 = d0 - d7, t6 = d1 - d6, t5 = d2 - d5, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = kRowPass ? 11 : 15;
    d[0] = kRowPass ? (t10 + t11) * 4 : jpeg_descale(t10 + t11, 2);
    d[4 * stride] = kRowPass ? (t10 - t11) * 4 : jpeg_descale(t10 - t11, 2);
    const int z1 = (t12 + t13) * 4433;
    d[2 * stride] = jpeg_descale(z1 + t13 * 6270, n);
    d[6 * stride] = jpeg_descale(z1 - t12 * 15137, n);
    int o[4];
    jpeg_odd_part(t4, t5, t6, t7, o);
    d[7 * stride] = jpeg_descale(o[0], n);
    d[5 * stride] = jpeg_descale(o[1], n);
    d[3 * stride] = jpeg_descale(o[2], n);
    d[stride] = jpeg_descale(o[3], n);
}
// One inverse pass; n: 11 (columns) or 18 (rows).
template <int n>
SX_JPEG_FN void jpeg_inverse_pass(int* c, int stride) {
    const int c0 = c[0], c1 = c[stride], c2 = c[2 * stride], c3 = c[3 * stride], c4 = c[4 * stride], c5 = c[5 * stride], c6 = c[6 * stride], c7 = c[7 * stride];
    const int z1 = (c2 + c6) * 4433;
    const int t2 = z1 - c6 * 15137, t3 = z1 + c2 * 6270;
    const int t0 = (c0 + c4) * 8192, t1 = (c0 - c4) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o[4];
    jpeg_odd_part(c7, c5, c3, c1, o);
    c[0] = jpeg_descale(t10 + o[3], n);
    c[7 * stride] = jpeg_descale(t10 - o[3], n);
    c[stride] = jpeg_descale(t11 + o[2], n);
    c[6 * stride] = jpeg_descale(t11 - o[2], n);
    c[2 * stride] = jpeg_descale(t12 + o[1], n);
    c[5 * stride] = jpeg_descale(t12 - o[1], n);
    c[3 * stride] = jpeg_descale(t13 + o[0], n);
    c[4 * stride] = jpeg_descale(t13 - o[0], n);
}
// v: a block in row-major order, level - 128 -> the coefficients times 8.  Rows, then columns.
SX_JPEG_FN void jpeg_forward_dct(int (&v)[64]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) jpeg_forward_pass<true>(v + 8 * r, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) jpeg_forward_pass<false>(v + c, 8);
}
// v: the dequantised coefficients -> the levels 0..255.  Columns, then rows.
SX_JPEG_FN void jpeg_inverse_dct(int (&v)[64]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) jpeg_inverse_pass<11>(v + c, 8);
#pragma unroll
    for (int r = 0; r < 8; ++r) jpeg_inverse_pass<18>(v + 8 * r, 1);
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = jpeg_clamp(v[i] + 128, 0, 255);
}
// A block through the codec: levels in, levels out.  q / magic: the 64 table entries of the block's plane and their jpeg_magic().
template <typename Q, typename M>
SX_JPEG_FN void jpeg_code_block(int (&v)[64], const Q* q, const M* magic) {
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] -= 128;
    jpeg_forward_dct(v);
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = jpeg_requantise(v[i], (int)q[i], (uint32_t)magic[i]);
    jpeg_inverse_dct(v);
}

// ---- 4:2:0 --------------------------------------------------------------------------------------------------------------------------------
// The 2 x 2 mean of chroma sample (., cx): bias 1 in even output columns, 2 in odd ones.
SX_JPEG_FN int jpeg_chroma_mean(int a, int b, int c, int d, int cx) { return (a + b + c + d + 1 + (cx & 1)) >> 2; }
// Four neighbouring output pixels (columns 2 cx .. 2 cx + 3) of one output row through the triangle filter.  near[k] / other[k]: the
// decoded chroma samples of the row's own chroma row and of the row above (upper output row of a pair) or below (lower), at chroma
// columns cx - 1, cx, cx + 1, cx + 2, each clamped into the plane.  `replicate`: the plane is at most two columns wide -- no filter.
SX_JPEG_FN void jpeg_chroma_up4(const int (&near)[4], const int (&other)[4], bool replicate, int (&out)[4]) {
    if (replicate) {
        out[0] = out[1] = near[1];
        out[2] = out[3] = near[2];
        return;
    }
    int t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = 3 * near[k] + other[k];
    out[0] = (3 * t[1] + t[0] + 8) >> 4;
    out[1] = (3 * t[1] + t[2] + 7) >> 4;
    out[2] = (3 * t[2] + t[1] + 8) >> 4;
    out[3] = (3 * t[2] + t[3] + 7) >> 4;
}

// ---- the index arithmetic: a tile of `height` x `width` pixels, a region at (y0, x0), `sub` 0 (4:4:4) or 2 (4:2:0) -------------------------
struct JpegRegion {
    int height, width, sub;
    int y0, x0;                // the region's first pixel: multiples of region_h() / kJpegRegionW
    SX_JPEG_MEMBER int region_h() const { return sub ? kJpegRegionH420 : kJpegRegionH444; }
    SX_JPEG_MEMBER int rows_in() const { const int r = height - y0; return r < region_h() ? r : region_h(); }                  // pixels of the tile in the region
    SX_JPEG_MEMBER int cols_in() const { const int c = width - x0; return c < kJpegRegionW ? c : kJpegRegionW; }
    SX_JPEG_MEMBER int rows_coded() const { return (rows_in() + 7) & ~7; }                                                   // ... extended to whole blocks
    SX_JPEG_MEMBER int cols_coded() const { return (cols_in() + 7) & ~7; }
    // full-resolution planes: the source pixel of coded row / column `l` of the region (the last row / column replicated)
    SX_JPEG_MEMBER int source_row(int l) const { const int y = y0 + l; return y < height ? y : height - 1; }
    SX_JPEG_MEMBER int source_col(int l) const { const int x = x0 + l; return x < width ? x : width - 1; }
    // 4:2:0: the chroma plane is chroma_h() x chroma_w() samples in 8 x 8 blocks; the window on chip starts kJpegHalo samples before the
    // region's first sample and holds the samples [win_lo, win_hi) of each axis, window-local: whole blocks that exist
    SX_JPEG_MEMBER int chroma_h() const { return (height + 1) >> 1; }
    SX_JPEG_MEMBER int chroma_w() const { return (width + 1) >> 1; }
    SX_JPEG_MEMBER int win_y() const { return (y0 >> 1) - kJpegHalo; }
    SX_JPEG_MEMBER int win_x() const { return (x0 >> 1) - kJpegHalo; }
    SX_JPEG_MEMBER static int lo_of(int win) { return win < 0 ? -win : 0; }
    SX_JPEG_MEMBER static int hi_of(int win, int samples) { const int coded = (samples + 7) & ~7; return coded - win < kJpegChromaSide ? coded - win : kJpegChromaSide; }
    SX_JPEG_MEMBER int win_lo_y() const { return lo_of(win_y()); }
    SX_JPEG_MEMBER int win_lo_x() const { return lo_of(win_x()); }
    SX_JPEG_MEMBER int win_hi_y() const { return hi_of(win_y(), chroma_h()); }
    SX_JPEG_MEMBER int win_hi_x() const { return hi_of(win_x(), chroma_w()); }
    // the two source rows of chroma row `cy` (plane coordinates): the bottom row replicated to an even height, then the last
    // DOWNSAMPLED row replicated; the two source columns of chroma column `cx`: the last column replicated
    SX_JPEG_MEMBER void chroma_rows(int cy, int (&rows)[2]) const {
        const int c = cy < chroma_h() ? cy : chroma_h() - 1;
        rows[0] = 2 * c;      // (2 (chroma_h - 1) <= height - 1)
        rows[1] = 2 * c + 1 < height ? 2 * c + 1 : height - 1;
    }
    SX_JPEG_MEMBER int chroma_col(int x) const { return x < width ? x : width - 1; }      // x = 2 cx, 2 cx + 1
    // the filter's reads for output row y (plane coordinates): its own chroma row and the other one, clamped into the plane
    SX_JPEG_MEMBER int up_row(int y) const { return y >> 1; }
    SX_JPEG_MEMBER int up_other_row(int y) const {
        const int cy = y >> 1;
        return (y & 1) ? (cy + 1 < chroma_h() ? cy + 1 : chroma_h() - 1) : (cy > 0 ? cy - 1 : 0);
    }
    // ... and its four columns for the output pixels 2 cx .. 2 cx + 3: cx - 1, cx, cx + 1, cx + 2 clamped into the plane
    SX_JPEG_MEMBER int up_col(int cx, int k) const { return jpeg_clamp(cx - 1 + k, 0, chroma_w() - 1); }
    // the blocks a workgroup codes: job j of jobs().  -> the byte offset of the block's first sample in the planes' storage, the row pitch
    // and whether the chrominance table applies; false: the block does not exist in this region
    SX_JPEG_MEMBER int jobs() const { return sub ? (kJpegRegionH420 / 8) * (kJpegRegionW / 8) + 2 * (kJpegChromaSide / 8) * (kJpegChromaSide / 8) : 3 * (kJpegRegionH444 / 8) * (kJpegRegionW / 8); }
    SX_JPEG_MEMBER bool job(int j, int& offset, int& pitch, int& chroma) const {
        constexpr int kAcross = kJpegRegionW / 8, kFull444 = (kJpegRegionH444 / 8) * kAcross, kFull420 = (kJpegRegionH420 / 8) * kAcross, kSide = kJpegChromaSide / 8;
        if (sub == 0 || j < kFull420) {
            const int plane = sub ? 0 : j / kFull444, k = sub ? j : j % kFull444, by = k / kAcross, bx = k % kAcross;
            offset = plane * kJpegPlaneBytes444 + 8 * by * kJpegPitch + 8 * bx;      // (4:2:0: plane 0)
            pitch = kJpegPitch;
            chroma = plane != 0;
            return 8 * by < rows_coded() && 8 * bx < cols_coded();
        }
        const int k = j - kFull420, plane = k / (kSide * kSide), by = (k % (kSide * kSide)) / kSide, bx = k % kSide;
        offset = kJpegLumaBytes420 + plane * kJpegChromaBytes420 + 8 * by * kJpegChromaPitch + 8 * bx;
        pitch = kJpegChromaPitch;
        chroma = 1;
        return 8 * by >= win_lo_y() && 8 * by < win_hi_y() && 8 * bx >= win_lo_x() && 8 * bx < win_hi_x();
    }
};

}  // namespace jpeg_block
}  // namespace sx

#undef SX_JPEG_FN
#undef SX_JPEG_MEMBER

#endif  // SX_JPEG_BLOCK_HPP
