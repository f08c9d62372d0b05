// Host check of the JPEG round trip's block and index arithmetic (stainx_amd/csrc/jpeg_block.hpp: the very functions the kernel calls).
//   1. The quantiser's reciprocal multiplication against plain `/` for every divisor 8 Q, Q in 1..255, and every numerator |c| + 4 Q with
//      |c| up to 2^17 -- sixteen times the bound on a coefficient that is derived and printed first.
//   2. No intermediate of the two transforms overflows int32 (the undefined-behaviour sanitizer watches every signed operation): blocks of
//      extreme levels -- flat, the 64 sign patterns that maximise each coefficient, both polarities, random 0 / 255 -- and random levels,
//      through jpeg_code_block with tables of all 1 and all 255 and with the tables of qualities 1, 50 and 100.  The largest coefficient
//      met is printed beside the bound.
//   3. The kernel's three sweeps walked region by region as the kernel walks them, for every H, W in 1..40, 63..65 and 127..130 and both
//      subsamplings: every source pixel inside the tile, every byte of the on-chip planes inside the array (a vector of EXACTLY
//      kJpegPlaneBytes bytes, so that the address sanitizer sees every access), every block the codec reads written whole by the colour
//      sweep, every sample the output sweep reads decoded, every pixel of the tile written exactly once.
// No GPU, no HIP: build with the host compiler and the sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=undefined,address -fno-sanitize-recover=all tools/jpeg_block_check.cpp -o jpeg_block_check && ./jpeg_block_check
// It prints what it checked and exits 0, or names the first failure and exits 1.
#include "../stainx_amd/csrc/jpeg_block.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace sx::jpeg_block;

[[noreturn]] static void fail(const char* what, long long a, long long b, long long c, long long d) {
    std::fprintf(stderr, "FAIL %s: %lld %lld %lld %lld\n", what, a, b, c, d);
    std::exit(1);
}

// ---- 1. the bound and the quantiser -----------------------------------------------------------------------------------------------------
static int coefficient_bound() {
    // A pass is out_k = sum_x d_x a_k(x) with a_0 = 1 and a_k(x) = sqrt(2) cos((2 x + 1) k pi / 16): the largest sum of |a_k(x)| is 8, at k = 0.
    const double pi = std::acos(-1.0);
    double gain = 0.0;
    for (int k = 0; k < 8; ++k) {
        double s = 0.0;
        for (int x = 0; x < 8; ++x) s += std::fabs(k == 0 ? 1.0 : std::sqrt(2.0) * std::cos((2 * x + 1) * k * pi / 16.0));
        gain = s > gain ? s : gain;
    }
    // |level - 128| <= 128; the row pass multiplies by 4 and rounds (+ 1), the column pass divides by 4 and rounds (+ 1); the twelve 13-bit
    // constants are off by at most 2^-14 each of a sum of at most four products (+ 1 %, generous).
    const double rows = gain * 4.0 * 128.0 * 1.01 + 1.0;
    return (int)std::ceil(gain * rows / 4.0 * 1.01 + 1.0);
}

static void check_quantiser(int bound) {
    const int limit = 1 << 17;
    if (16 * bound > limit + 4096) fail("the quantiser's sweep does not cover the bound", bound, limit, 0, 0);
    unsigned long long checked = 0;
    for (int q = 1; q <= 255; ++q) {
        const uint32_t d = 8u * (uint32_t)q, magic = jpeg_magic(q);
        for (int c = 0; c <= limit; ++c) {
            const uint32_t n = (uint32_t)c + 4u * (uint32_t)q;
            if (jpeg_divide(n, magic) != (int)(n / d)) fail("jpeg_divide", q, c, jpeg_divide(n, magic), n / d);
            ++checked;
        }
        for (int c : {-limit, -bound, -9, -8, -7, -1, 0, 1, 7, 8, 9, bound, limit}) {
            const int mag = c < 0 ? -c : c, want = (mag + ((8 * q) >> 1)) / (8 * q) * q;
            if (jpeg_requantise(c, q, magic) != (c < 0 ? -want : want)) fail("jpeg_requantise", q, c, jpeg_requantise(c, q, magic), want);
        }
    }
    std::printf("quantiser: %llu quotients equal to plain division (Q 1..255, |c| 0..%d = 2^17); derived bound on |c|: %d\n", checked, limit, bound);
}

// ---- 2. the transforms -------------------------------------------------------------------------------------------------------------------
static int largest_coefficient = 0;
static unsigned long long blocks_coded = 0;

static void code_with(const int (&levels)[64], const int* q) {
    uint32_t magic[64];
    for (int i = 0; i < 64; ++i) magic[i] = jpeg_magic(q[i]);
    int v[64], c[64];
    for (int i = 0; i < 64; ++i) v[i] = levels[i], c[i] = levels[i] - 128;
    jpeg_forward_dct(c);
    for (int i = 0; i < 64; ++i) largest_coefficient = std::abs(c[i]) > largest_coefficient ? std::abs(c[i]) : largest_coefficient;
    jpeg_code_block(v, q, magic);
    for (int i = 0; i < 64; ++i)
        if (v[i] < 0 || v[i] > 255) fail("a decoded level outside 0..255", i, v[i], 0, 0);
    ++blocks_coded;
}

static void check_transforms(int bound) {
    int tables[5][64];
    for (int i = 0; i < 64; ++i) tables[0][i] = 1, tables[1][i] = 255, tables[2][i] = jpeg_table_entry(1, 0, i), tables[3][i] = jpeg_table_entry(50, 1, i), tables[4][i] = jpeg_table_entry(100, 0, i);
    auto all_tables = [&](const int (&levels)[64]) {
        for (auto& t : tables) code_with(levels, t);
    };
    const double pi = std::acos(-1.0);
    int levels[64];
    for (int flat : {0, 1, 127, 128, 129, 254, 255}) {
        for (int& l : levels) l = flat;
        all_tables(levels);
    }
    for (int u = 0; u < 8; ++u)
        for (int v = 0; v < 8; ++v)
            for (int polarity = 0; polarity < 2; ++polarity) {      // the block that maximises coefficient (u, v)
                for (int y = 0; y < 8; ++y)
                    for (int x = 0; x < 8; ++x) {
                        const bool up = std::cos((2 * y + 1) * u * pi / 16.0) * std::cos((2 * x + 1) * v * pi / 16.0) >= 0.0;
                        levels[8 * y + x] = (up != (polarity != 0)) ? 255 : 0;
                    }
                all_tables(levels);
            }
    std::mt19937 rng(20261021u);
    for (int round = 0; round < 20000; ++round) {
        for (int& l : levels) l = (rng() & 1u) ? 255 : 0;
        all_tables(levels);
        for (int& l : levels) l = (int)(rng() & 255u);
        all_tables(levels);
    }
    if (largest_coefficient > bound) fail("a coefficient above the derived bound", largest_coefficient, bound, 0, 0);
    std::printf("transforms: %llu blocks through both transforms with no int32 overflow; largest |coefficient| met %d (bound %d)\n", blocks_coded, largest_coefficient, bound);
}

// ---- 3. the sweeps --------------------------------------------------------------------------------------------------------------------------
static unsigned long long source_reads = 0, plane_accesses = 0, regions_walked = 0;
enum : unsigned char { kUnwritten = 0, kColour = 1, kDecoded = 2 };

static void walk_tile(int height, int width, int sub) {
    std::vector<unsigned char> written((size_t)height * width, 0);
    const int region_h = sub ? kJpegRegionH420 : kJpegRegionH444;
    for (int y0 = 0; y0 < height; y0 += region_h)
        for (int x0 = 0; x0 < width; x0 += kJpegRegionW) {
            JpegRegion g{height, width, sub, y0, x0};
            std::vector<unsigned char> planes(kJpegPlaneBytes, kUnwritten);      // (.at(): a second check beside the sanitizer's)
            auto source = [&](int row, int col) {
                if (row < 0 || row >= height || col < 0 || col >= width) fail("a source pixel outside the tile", height, width, row, col);
                ++source_reads;
            };
            auto mark = [&](int at, int bytes, unsigned char state, unsigned char expect) {
                for (int b = 0; b < bytes; ++b) {
                    if (planes.at((size_t)(at + b)) != expect) fail("a plane byte in the wrong state", height, width, at + b, planes.at((size_t)(at + b)));
                    planes.at((size_t)(at + b)) = state;
                    ++plane_accesses;
                }
            };
            // 1. colour
            const int rows_coded = g.rows_coded(), quads_coded = g.cols_coded() / 4;
            if (rows_coded > region_h || g.cols_coded() > kJpegRegionW) fail("a region larger than its planes", height, width, rows_coded, g.cols_coded());
            for (int i = 0; i < rows_coded * quads_coded; ++i) {
                const int lr = i / quads_coded, lx = 4 * (i % quads_coded);
                for (int e = 0; e < 4; ++e) source(g.source_row(lr), g.x0 + lx + 3 < width ? g.x0 + lx + e : g.source_col(lx + e));
                for (int plane = 0; plane < (sub ? 1 : 3); ++plane) mark(plane * kJpegPlaneBytes444 + lr * kJpegPitch + lx, 4, kColour, kUnwritten);
            }
            if (sub) {
                const int lo_y = g.win_lo_y(), lo_x = g.win_lo_x(), rows = g.win_hi_y() - lo_y, span = g.win_hi_x() - lo_x;
                if (lo_y % 8 || lo_x % 8 || rows % 8 || span % 8 || rows <= 0 || span <= 0) fail("a chroma window that is not whole blocks", height, width, rows, span);
                for (int i = 0; i < rows * (span / 2); ++i) {
                    const int ly = lo_y + i / (span / 2), lx = lo_x + 2 * (i % (span / 2)), x = 2 * (g.win_x() + lx);
                    if (g.win_y() + ly < 0 || x < 0) fail("a chroma sample before the plane", height, width, ly, lx);
                    int rows2[2];
                    g.chroma_rows(g.win_y() + ly, rows2);
                    for (int r = 0; r < 2; ++r)
                        for (int e = 0; e < 4; ++e) source(rows2[r], x + 3 < width ? x + e : g.chroma_col(x + e));
                    for (int plane = 0; plane < 2; ++plane) mark(kJpegLumaBytes420 + plane * kJpegChromaBytes420 + ly * kJpegChromaPitch + lx, 2, kColour, kUnwritten);
                }
            }
            // 2. blocks
            for (int j = 0; j < g.jobs(); ++j) {
                int offset, pitch, chroma;
                if (!g.job(j, offset, pitch, chroma)) continue;
                if (offset % 8 || pitch % 8) fail("a block row that is not an aligned word", height, width, offset, pitch);
                for (int r = 0; r < 8; ++r) mark(offset + r * pitch, 8, kDecoded, kColour);
            }
            for (size_t b = 0; b < planes.size(); ++b)
                if (planes[b] == kColour) fail("a plane byte converted but never coded", height, width, (long long)b, sub);
            // 3. output
            const int rows_in = g.rows_in(), cols_in = g.cols_in(), quads = (cols_in + 3) / 4;
            auto decoded = [&](int at) {
                if (planes.at((size_t)at) != kDecoded) fail("the output sweep reads a byte that was not decoded", height, width, at, sub);
                ++plane_accesses;
            };
            for (int i = 0; i < rows_in * quads; ++i) {
                const int lr = i / quads, lx = 4 * (i % quads);
                for (int e = 0; e < 4; ++e)
                    for (int plane = 0; plane < (sub ? 1 : 3); ++plane) decoded(plane * kJpegPlaneBytes444 + lr * kJpegPitch + lx + e);
                if (sub) {
                    const int y = g.y0 + lr, cx = (g.x0 + lx) >> 1;
                    for (int row : {g.up_row(y), g.up_other_row(y)})
                        for (int k = 0; k < 4; ++k) {
                            const int col = g.up_col(cx, k);
                            if (row < 0 || row >= g.chroma_h() || col < 0 || col >= g.chroma_w()) fail("the filter reads outside the cropped chroma plane", height, width, row, col);
                            const int ly = row - g.win_y(), lc = col - g.win_x();
                            if (ly < 0 || ly >= kJpegChromaSide || lc < 0 || lc >= kJpegChromaSide) fail("the filter reads outside the chroma window", height, width, ly, lc);
                            for (int plane = 0; plane < 2; ++plane) decoded(kJpegLumaBytes420 + plane * kJpegChromaBytes420 + ly * kJpegChromaPitch + lc);
                        }
                }
                for (int e = 0; e < 4; ++e)
                    if (g.x0 + lx + e < width) ++written.at((size_t)(g.y0 + lr) * width + g.x0 + lx + e);
            }
            ++regions_walked;
        }
    for (size_t p = 0; p < written.size(); ++p)
        if (written[p] != 1) fail("a pixel not written exactly once", height, width, (long long)p, written[p]);
}

int main() {
    const int bound = coefficient_bound();
    check_quantiser(bound);
    check_transforms(bound);
    std::vector<int> sizes;
    for (int s = 1; s <= 40; ++s) sizes.push_back(s);
    for (int s : {63, 64, 65, 127, 128, 129, 130, 255, 256, 257}) sizes.push_back(s);
    for (int h : sizes)
        for (int w : sizes)
            for (int sub : {0, 2}) walk_tile(h, w, sub);
    std::printf("sweeps: %zu x %zu shapes x 2 subsamplings, %llu regions: %llu source reads inside their tiles, %llu plane accesses inside %d bytes, every block whole, every pixel written once\n",
                sizes.size(), sizes.size(), regions_walked, source_reads, plane_accesses, kJpegPlaneBytes);
    std::printf("OK\n");
    return 0;
}
