// Host check of the affine warp's index arithmetic (stainx_amd/csrc/warp.hpp: warp_effective_row, warp_coord, warp_fold, warp_axis,
// warp_taps -- the very functions the kernel calls; warp_coord is the kernel's fmaf(a, x, fmaf(b, y, c)), whose inner term the kernel
// shares among a thread's four pixels): rows of every kind are swept over shapes from 1 x 1 to 144 x 128 and every tap
// position is asserted to lie inside the source plane, every axis index in [0, n).  No GPU, no HIP: build with the host compiler and
// the sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=undefined,address -fno-sanitize-recover=all tools/warp_index_check.cpp -o warp_index_check && ./warp_index_check
// It prints the number of taps checked and exits 0, or names the first row, shape and pixel that fails and exits 1.
#define SX_WARP_INDEX_ONLY
#include "../stainx_amd/csrc/warp.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace sx::warp_index;

struct Shape { int64_t h, w, oh, ow; };

static float bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static unsigned long long checked = 0;

[[noreturn]] static void fail(const char* what, const float (&row)[6], const Shape& s, int64_t x, int64_t y, long long got) {
    std::fprintf(stderr, "FAIL %s: got %lld; row (%g, %g, %g, %g, %g, %g), source %lld x %lld, output %lld x %lld, pixel (x %lld, y %lld)\n", what, got, row[0], row[1], row[2], row[3],
                 row[4], row[5], (long long)s.h, (long long)s.w, (long long)s.oh, (long long)s.ow, (long long)x, (long long)y);
    std::exit(1);
}

static void sweep(const float (&given)[6], const Shape& s) {
    float row[6];
    const bool anchor = warp_effective_row(given, s.h, s.w, s.oh, s.ow, row);
    for (int k = 0; k < 6; ++k)
        if (!(std::fabs(row[k]) < std::numeric_limits<float>::infinity())) fail("the row in use is not finite", given, s, 0, 0, k);
    if (anchor && (row[0] != 1.0f || row[1] != 0.0f || row[3] != 0.0f || row[4] != 1.0f || 2 * (int64_t)row[2] > s.w - s.ow || 2 * (int64_t)row[2] < s.w - s.ow - 1
                   || 2 * (int64_t)row[5] > s.h - s.oh || 2 * (int64_t)row[5] < s.h - s.oh - 1))
        fail("the anchor row", given, s, 0, 0, (long long)row[2]);
    const uint64_t plane = (uint64_t)s.h * (uint64_t)s.w;
    for (int64_t y = 0; y < s.oh; ++y) {
        for (int64_t x = 0; x < s.ow + 3; ++x) {      // (the kernel computes up to three columns past the edge of a ragged block)
            const float sx = warp_coord(row[0], row[1], row[2], (float)x, (float)y), sy = warp_coord(row[3], row[4], row[5], (float)x, (float)y);
            const bool ok = warp_coord_ok(sx) && warp_coord_ok(sy);
            for (int mode = 0; mode < 4; ++mode) {
                const bool nearest = (mode & 1) != 0, constant = (mode & 2) != 0;
                const WarpTaps t = warp_taps(sx, sy, nearest, constant, s.h, s.w);
                for (int k = 0; k < 4; ++k) {
                    if ((uint64_t)t.at[k] >= plane) fail("a tap position outside the plane", given, s, x, y, (long long)t.at[k]);
                    ++checked;
                }
                if (!ok && (t.outside != 0xFu || t.fx != 0.0f || t.fy != 0.0f)) fail("a coordinate past the limit must be all fill", given, s, x, y, t.outside);
                if (ok && !constant && t.outside != 0u) fail("a mirrored tap marked as fill", given, s, x, y, t.outside);
                if (!(t.fx >= 0.0f && t.fx <= 1.0f && t.fy >= 0.0f && t.fy <= 1.0f)) fail("a fraction outside [0, 1]", given, s, x, y, -1);      // (1 for a negative coordinate tinier than 2^-25: s - floor(s) rounds)
                if (nearest && (t.fx != 0.0f || t.fy != 0.0f)) fail("nearest with a fraction", given, s, x, y, -1);
                if (ok) {      // the axes on their own: every index in [0, n)
                    const float ax = nearest ? floorf(sx + 0.5f) : sx, ay = nearest ? floorf(sy + 0.5f) : sy;
                    int xs[2], ys[2];
                    unsigned ox, oy;
                    warp_axis(ax, constant, s.w, xs, ox);
                    warp_axis(ay, constant, s.h, ys, oy);
                    for (int k = 0; k < 2; ++k) {
                        if (xs[k] < 0 || xs[k] >= s.w) fail("an x index outside [0, W)", given, s, x, y, xs[k]);
                        if (ys[k] < 0 || ys[k] >= s.h) fail("a y index outside [0, H)", given, s, x, y, ys[k]);
                    }
                    if (!constant) {      // the fold against the definition: walk from 0, turning at the ends
                        const int q0 = (int)floorf(ax);
                        if (std::abs(q0) <= 4096 && s.w > 1) {
                            const int64_t period = 2 * (s.w - 1);
                            int64_t m = ((q0 % period) + period) % period;
                            m = m >= s.w ? period - m : m;
                            if (xs[0] != m) fail("the fold disagrees with its definition", given, s, x, y, xs[0]);
                        }
                    }
                }
            }
        }
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = SX_WARP_MAX_COORD;
    const float denormal = bits(1u), small = 1e-30f, huge = 1e30f, maxf = std::numeric_limits<float>::max();
    // the values a row entry takes, one at a time, in an otherwise ordinary row
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.5f, 0.25f, 1.0f / 3.0f, 0.70710678f, -0.70710678f, 1.9f, -7.3f, 100.0f, -1000.0f, 65536.0f, -65536.0f, big, -big,
                             std::nextafter(big, inf), std::nextafter(big, 0.0f), -std::nextafter(big, inf), big - 1.0f, big - 0.5f, big + 1.0f, 2.0f * big, -2.0f * big,
                             8388608.0f, 16777216.0f, 2147483648.0f, -2147483648.0f, 4294967296.0f, 9.3e18f, -9.3e18f, huge, -huge, maxf, -maxf, small, -small, denormal, -denormal,
                             bits(0x007FFFFFu), nan, -nan, bits(0x7FC00001u), bits(0xFFFFFFFFu), inf, -inf};
    const int n_special = (int)(sizeof(special) / sizeof(special[0]));
    std::vector<Shape> shapes;
    const int64_t sides[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 2}, {5, 3}, {8, 8}, {33, 31}, {64, 64}, {65, 130}, {144, 128}};
    for (const auto& s : sides) shapes.push_back({s[0], s[1], s[0], s[1]});
    for (const Shape extra : {Shape{33, 31, 17, 40}, Shape{33, 31, 40, 40}, Shape{64, 64, 24, 24}, Shape{1, 1, 5, 9}, Shape{5, 3, 1, 1}, Shape{2, 2, 33, 35}, Shape{144, 128, 31, 33},
                              Shape{7, 1, 2, 64}, Shape{16, 16, 15, 17}})
        shapes.push_back(extra);

    const float ordinary[][6] = {{1, 0, 0, 0, 1, 0}, {1, 0, 0.25f, 0, 1, 0.25f}, {0, -1, 30, 1, 0, 0}, {-1, 0, 30, 0, 1, 0}, {0.8660254f, -0.5f, 3.1f, 0.5f, 0.8660254f, -2.2f},
                                 {0.70710678f, -0.70710678f, 16, 0.70710678f, 0.70710678f, -8}, {0.5f, 0, 0.5f, 0, 0.5f, 0.5f}, {1.9f, 0.3f, -40, -0.2f, 1.7f, 90},
                                 {1, 0, 1000.25f, 0, 1, -777.5f}, {0.75f, -0.5f, 3.0625f, 0.5f, 0.75f, -2.1875f}, {1, 0, -0.5f, 0, 1, 0.5f}, {3, 3, -300, -3, 3, 300}};
    for (const Shape& s : shapes) {
        for (const auto& row : ordinary) sweep(row, s);
        const bool large = s.oh * s.ow > 4096;
        for (int k = 0; k < 6; ++k) {      // every special value in every place of a rotation row ...
            for (int i = 0; i < n_special; ++i) {
                float row[6] = {0.8660254f, -0.5f, 3.1f, 0.5f, 0.8660254f, -2.2f};
                row[k] = special[i];
                sweep(row, s);
                if (large) continue;
                for (int j = 0; j < n_special; j += 3) {      // ... and pairs of them, in this place and the next
                    row[(k + 1) % 6] = special[j];
                    sweep(row, s);
                }
            }
        }
        for (int i = 0; i < n_special; ++i) {      // all six the same special value, and the identity with a special offset on both axes
            const float all[6] = {special[i], special[i], special[i], special[i], special[i], special[i]};
            sweep(all, s);
            const float shift[6] = {1, 0, special[i], 0, 1, special[i]};
            sweep(shift, s);
        }
        // the coordinate limit from both sides, on the first and on the last pixel of the axis
        for (const float at : {big, std::nextafter(big, inf), std::nextafter(big, 0.0f), big - 0.5f, big - 0.25f}) {
            for (const float sign : {1.0f, -1.0f}) {
                const float first[6] = {1, 0, sign * at, 0, 1, sign * at};
                sweep(first, s);
                const float last[6] = {1, 0, sign * at - (float)(s.ow - 1), 0, 1, sign * at - (float)(s.oh - 1)};
                sweep(last, s);
                const float slope[6] = {sign * at / (float)s.ow, 0, 0, 0, sign * at / (float)s.oh, 0};
                sweep(slope, s);
            }
        }
    }
    // axes longer than any index within the limit (no memory is touched: the functions alone): one reflection at 0, never past n
    for (const int64_t n : {(int64_t)kWarpFoldDirect - 1, (int64_t)kWarpFoldDirect, (int64_t)kWarpFoldDirect + 1, (int64_t)1 << 31, ((int64_t)1 << 32) - 1}) {
        for (const int q : {-(1 << 22) - 1, -(1 << 22), -1, 0, 1, (1 << 22), (1 << 22) + 1}) {
            const int m = warp_fold(q, n);
            if (m < 0 || m >= n || m != std::abs(q)) {
                std::fprintf(stderr, "FAIL warp_fold(%d, %lld) = %d\n", q, (long long)n, m);
                return 1;
            }
            ++checked;
        }
    }
    // the anchor offsets: floor division for odd differences in both directions
    if (warp_anchor_offset(10, 7) != 1.0f || warp_anchor_offset(7, 10) != -2.0f || warp_anchor_offset(8, 8) != 0.0f || warp_anchor_offset(9, 8) != 0.0f || warp_anchor_offset(8, 9) != -1.0f) {
        std::fprintf(stderr, "FAIL warp_anchor_offset\n");
        return 1;
    }
    std::printf("warp_index_check: %llu tap positions and fold results inside their bounds, %zu shapes\n", checked, shapes.size());
    return 0;
}
