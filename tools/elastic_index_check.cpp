// Host check of the elastic warp's index arithmetic (stainx_amd/csrc/elastic.hpp: elastic_grid_dim, elastic_cell, elastic_block_span,
// elastic_local, elastic_weights, elastic_sum -- the very functions the kernel calls -- and warp.hpp's warp_effective_row, warp_coord,
// warp_taps).  The kernel's three steps are walked block by block as the kernel walks them: the control points a 32 x 32 block stages
// (read from a vector of EXACTLY 2 x GH x GW floats, so that the address sanitizer sees every read), the x pass over all 32 columns of
// the block -- the columns past the tile's edge included --, the y pass of every row, the add and warp_taps.  Cells 4, 5, 7, 16, 31,
// 32, 33, 64 and 4096, tools/warp_index_check.cpp's shapes, grids filled with its 48 special floats, its special rows.  Asserted: every
// control index inside the grid, every staged span within kElasticSpan, every local index within its span, every tap position inside
// the plane, a zero grid's taps equal to the affine warp's.  No GPU, no HIP: build with the host compiler and the sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=undefined,address -fno-sanitize-recover=all tools/elastic_index_check.cpp -o elastic_index_check && ./elastic_index_check
// It prints the numbers of control reads and taps checked and exits 0, or names the first cell, shape and pixel that fails and exits 1.
#define SX_WARP_INDEX_ONLY
#include "../stainx_amd/csrc/elastic.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace sx::warp_index;
using namespace sx::elastic_index;

struct Shape { int64_t h, w, oh, ow; };
constexpr int kSide = 32;      // the kernel's output block (warp.hpp: kWarpSide)

static float bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static unsigned long long control_reads = 0, taps_checked = 0;

[[noreturn]] static void fail(const char* what, int cell, const Shape& s, int64_t x, int64_t y, long long got) {
    std::fprintf(stderr, "FAIL %s: got %lld; cell %d, source %lld x %lld, output %lld x %lld, pixel (x %lld, y %lld)\n", what, got, cell, (long long)s.h, (long long)s.w, (long long)s.oh,
                 (long long)s.ow, (long long)x, (long long)y);
    std::exit(1);
}

// One tile as the kernel takes it.  `grid`: 2 x GH x GW floats; `compare`: the taps must be those of the affine warp (a zero grid).
static void sweep(const float (&given)[6], const std::vector<float>& grid, int cell, const Shape& s, bool compare) {
    float row[6];
    const bool anchor = warp_effective_row(given, s.h, s.w, s.oh, s.ow, row);
    const int64_t gh = elastic_grid_dim(s.oh, cell), gw = elastic_grid_dim(s.ow, cell);
    if ((int64_t)grid.size() != 2 * gh * gw) fail("the grid's size", cell, s, 0, 0, (long long)grid.size());
    const uint64_t plane_size = (uint64_t)s.h * (uint64_t)s.w;
    float control[2][kElasticSpan][kElasticSpan], across[2][kElasticSpan][kSide];
    for (int64_t y0 = 0; y0 < s.oh; y0 += kSide) {
        for (int64_t x0 = 0; x0 < s.ow; x0 += kSide) {
            int first_row = 0, first_col = 0, n_rows = 0, n_cols = 0;
            if (!anchor) {      // (a tile that is left reads no grid)
                n_rows = elastic_block_span(y0, kSide, s.oh, cell, first_row);
                n_cols = elastic_block_span(x0, kSide, s.ow, cell, first_col);
                float unused;
                if (elastic_cell(y0 + kSide - 1, s.oh, cell, unused) - first_row + 4 > kElasticSpan) fail("a block's control rows exceed the span", cell, s, x0, y0, n_rows);
                if (elastic_cell(x0 + kSide - 1, s.ow, cell, unused) - first_col + 4 > kElasticSpan) fail("a block's control columns exceed the span", cell, s, x0, y0, n_cols);
                if (first_row < 0 || first_row + n_rows > gh) fail("staged control rows outside [0, GH)", cell, s, x0, y0, first_row + n_rows);
                if (first_col < 0 || first_col + n_cols > gw) fail("staged control columns outside [0, GW)", cell, s, x0, y0, first_col + n_cols);
                for (int i = 0; i < 2 * n_rows * n_cols; ++i) {
                    const int plane = i / (n_rows * n_cols), rest = i % (n_rows * n_cols), r = rest / n_cols, c = rest % n_cols;
                    control[plane][r][c] = grid.at((size_t)((plane * gh + first_row + r) * gw + first_col + c));
                    ++control_reads;
                }
                for (int i = 0; i < 2 * n_rows * kSide; ++i) {      // all 32 columns, past the tile's edge too
                    const int col = i % kSide, line = i / kSide, r = line % n_rows, plane = line / n_rows;
                    float t, w[4];
                    const int j_grid = elastic_cell(x0 + col, s.ow, cell, t), j = elastic_local(j_grid, first_col);
                    if (j_grid < 0 || j_grid + 3 >= gw) fail("a control column outside [0, GW)", cell, s, x0 + col, y0, j_grid);
                    if (j != j_grid - first_col || j < 0 || j + 3 >= n_cols) fail("a local control column outside its span", cell, s, x0 + col, y0, j);
                    if (!(t >= 0.0f && t < 1.0f)) fail("t outside [0, 1)", cell, s, x0 + col, y0, -1);
                    elastic_weights(t, w);
                    for (int k = 0; k < 4; ++k)
                        if (!(w[k] >= 0.0f && w[k] <= 1.0f)) fail("a weight outside [0, 1]", cell, s, x0 + col, y0, k);
                    if (x0 + col < s.ow && j_grid != (int)((x0 + col) / cell)) fail("jx is not x div cell", cell, s, x0 + col, y0, j_grid);
                    const float* p = control[plane][r];
                    across[plane][r][col] = elastic_sum(w, p[j], p[j + 1], p[j + 2], p[j + 3]);
                }
            }
            for (int r = 0; r < kSide && y0 + r < s.oh; ++r) {
                const int64_t gy = y0 + r;
                float ty = 0.0f, wy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                int j = 0;
                if (!anchor) {
                    const int j_grid = elastic_cell(gy, s.oh, cell, ty);
                    j = elastic_local(j_grid, first_row);
                    if (j_grid != (int)(gy / cell) || j_grid + 3 >= gh) fail("a control row outside [0, GH)", cell, s, x0, gy, j_grid);
                    if (j != j_grid - first_row || j < 0 || j + 3 >= n_rows) fail("a local control row outside its span", cell, s, x0, gy, j);
                    elastic_weights(ty, wy);
                }
                for (int col = 0; col < kSide; ++col) {      // (a thread computes four columns and stores fewer: up to the block's 32nd)
                    const int64_t gx = x0 + col;
                    float dx = 0.0f, dy = 0.0f;
                    if (!anchor) {
                        dx = elastic_sum(wy, across[0][j][col], across[0][j + 1][col], across[0][j + 2][col], across[0][j + 3][col]);
                        dy = elastic_sum(wy, across[1][j][col], across[1][j + 1][col], across[1][j + 2][col], across[1][j + 3][col]);
                    }
                    const float ax = warp_coord(row[0], row[1], row[2], (float)gx, (float)gy), ay = warp_coord(row[3], row[4], row[5], (float)gx, (float)gy);
                    const float sx = ax + dx, sy = ay + dy;
                    for (int mode = 0; mode < 4; ++mode) {
                        const bool nearest = (mode & 1) != 0, constant = (mode & 2) != 0;
                        const WarpTaps t = warp_taps(sx, sy, nearest, constant, s.h, s.w);
                        for (int k = 0; k < 4; ++k) {
                            if ((uint64_t)t.at[k] >= plane_size) fail("a tap position outside the plane", cell, s, gx, gy, (long long)t.at[k]);
                            ++taps_checked;
                        }
                        if (!(warp_coord_ok(sx) && warp_coord_ok(sy)) && (t.outside != 0xFu || t.fx != 0.0f || t.fy != 0.0f)) fail("a coordinate past the limit must be all fill", cell, s, gx, gy, t.outside);
                        if (compare) {
                            const WarpTaps u = warp_taps(ax, ay, nearest, constant, s.h, s.w);
                            if (std::memcmp(t.at, u.at, sizeof(t.at)) != 0 || t.outside != u.outside || t.fx != u.fx || t.fy != u.fy) fail("a zero grid moved a tap", cell, s, gx, gy, mode);
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
    // tools/warp_index_check.cpp's special floats: here the values of a grid, and of a row's offsets
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.5f, 0.25f, 1.0f / 3.0f, 0.70710678f, -0.70710678f, 1.9f, -7.3f, 100.0f, -1000.0f, 65536.0f, -65536.0f, big, -big,
                             std::nextafter(big, inf), std::nextafter(big, 0.0f), -std::nextafter(big, inf), big - 1.0f, big - 0.5f, big + 1.0f, 2.0f * big, -2.0f * big,
                             8388608.0f, 16777216.0f, 2147483648.0f, -2147483648.0f, 4294967296.0f, 9.3e18f, -9.3e18f, huge, -huge, maxf, -maxf, small, -small, denormal, -denormal,
                             bits(0x007FFFFFu), nan, -nan, bits(0x7FC00001u), bits(0xFFFFFFFFu), inf, -inf};
    const int n_special = (int)(sizeof(special) / sizeof(special[0]));
    static_assert(sizeof(special) / sizeof(special[0]) == 48, "the 48 special floats");
    std::vector<Shape> shapes;
    const int64_t sides[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 2}, {5, 3}, {8, 8}, {33, 31}, {64, 64}, {65, 130}, {144, 128}};
    for (const auto& s : sides) shapes.push_back({s[0], s[1], s[0], s[1]});
    for (const Shape extra : {Shape{33, 31, 17, 40}, Shape{33, 31, 40, 40}, Shape{64, 64, 24, 24}, Shape{1, 1, 5, 9}, Shape{5, 3, 1, 1}, Shape{2, 2, 33, 35}, Shape{144, 128, 31, 33},
                              Shape{7, 1, 2, 64}, Shape{16, 16, 15, 17}})
        shapes.push_back(extra);
    const float ordinary[][6] = {{1, 0, 0, 0, 1, 0}, {1, 0, 0.25f, 0, 1, 0.25f}, {0, -1, 30, 1, 0, 0}, {-1, 0, 30, 0, 1, 0}, {0.8660254f, -0.5f, 3.1f, 0.5f, 0.8660254f, -2.2f},
                                 {0.70710678f, -0.70710678f, 16, 0.70710678f, 0.70710678f, -8}, {0.5f, 0, 0.5f, 0, 0.5f, 0.5f}, {1.9f, 0.3f, -40, -0.2f, 1.7f, 90},
                                 {1, 0, 1000.25f, 0, 1, -777.5f}, {0.75f, -0.5f, 3.0625f, 0.5f, 0.75f, -2.1875f}, {1, 0, -0.5f, 0, 1, 0.5f}, {3, 3, -300, -3, 3, 300}};
    const float rotation[6] = {0.8660254f, -0.5f, 3.1f, 0.5f, 0.8660254f, -2.2f}, identity[6] = {1, 0, 0, 0, 1, 0};
    unsigned long long sweeps = 0;
    for (const int cell : {4, 5, 7, 16, 31, 32, 33, 64, 4096}) {
        for (const Shape& s : shapes) {
            const size_t count = (size_t)(2 * elastic_grid_dim(s.oh, cell) * elastic_grid_dim(s.ow, cell));
            std::vector<float> mixed(count), zero(count, 0.0f);      // every special in turn, so that neighbours differ; and the zero grid
            for (size_t i = 0; i < count; ++i) mixed[i] = special[(i * 7 + 3) % n_special];
            for (int i = 0; i < n_special; ++i) {      // a grid filled with one special float: an ordinary row, the identity, a special offset
                const std::vector<float> grid(count, special[i]);
                const float shift[6] = {1, 0, special[(i + 5) % n_special], 0, 1, special[(i + 11) % n_special]};
                sweep(rotation, grid, cell, s, false);
                sweep(identity, grid, cell, s, false);
                sweep(shift, grid, cell, s, false);
                sweeps += 3;
            }
            for (const auto& row : ordinary) {
                sweep(row, mixed, cell, s, false);
                sweep(row, zero, cell, s, true);
                sweeps += 2;
            }
            for (int i = 0; i < n_special; ++i) {      // the special rows: all six the same, a special offset, a special value in each place of a rotation
                const float all[6] = {special[i], special[i], special[i], special[i], special[i], special[i]};
                const float shift[6] = {1, 0, special[i], 0, 1, special[i]};
                float placed[6] = {0.8660254f, -0.5f, 3.1f, 0.5f, 0.8660254f, -2.2f};
                placed[i % 6] = special[i];
                sweep(all, mixed, cell, s, false);
                sweep(shift, mixed, cell, s, false);
                sweep(placed, mixed, cell, s, false);
                sweep(shift, zero, cell, s, true);
                sweeps += 4;
            }
        }
    }
    // the grid's size and the clamp at the largest axis the call accepts: indices only, no memory
    for (const int cell : {4, 4096}) {
        const int64_t on = ((int64_t)1 << 32) - 1, g = elastic_grid_dim(on, cell);
        for (const int64_t x : {(int64_t)0, on - 2, on - 1, on, on + 30}) {
            float t;
            const int j = elastic_cell(x, on, cell, t);
            if (j < 0 || j + 3 >= g || !(t >= 0.0f && t < 1.0f)) {
                std::fprintf(stderr, "FAIL elastic_cell(%lld, %lld, %d) = %d\n", (long long)x, (long long)on, cell, j);
                return 1;
            }
        }
    }
    if (elastic_grid_dim(512, 16) != 35 || elastic_grid_dim(1, 4) != 4 || elastic_grid_dim(4097, 4096) != 5 || elastic_grid_dim(33, 4096) != 4) {
        std::fprintf(stderr, "FAIL elastic_grid_dim\n");
        return 1;
    }
    std::printf("elastic_index_check: %llu control reads inside their grids and %llu tap positions inside their planes, %llu sweeps, %zu shapes, 9 cells\n", control_reads, taps_checked,
                sweeps, shapes.size());
    return 0;
}
