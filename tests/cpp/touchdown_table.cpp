// Stand-alone walk over the argument rules and the terrain lookup of include/hsddp_touchdown.h (cafe-mpc_amd/csrc/touchdown.hpp, pure host code):
// tests/test_touchdown_host.py builds it with -fsanitize=address,undefined and runs it on its own.  Every rule once, then lookups at the grid's
// corners, far outside it on every side and at a NaN, with exactly-sized buffers so that an index past the grid or the rows is an error.
// Prints "ok <checks>" and exits 0, or names the first failed check.
#define TOUCHDOWN_HOST_ONLY 1
#include "touchdown.hpp"
#include <cstdio>
#include <limits>
#include <vector>

static int n_checks = 0;
#define EXPECT(cond) do { n_checks++; if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
    using namespace hs;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const TdHandleInfo h{3, 5, 0}, h32{3, 5, 1};
    const TdPhaseInfo ph[3] = {{0, 2}, {0, 0}, {1, 0}};      // whole-body with two touchdown feet; whole-body without; single rigid body
    std::vector<double> ok(5 * 4, 0.01), bad = ok; bad[19] = nan;
    EXPECT(td_check_set(h, ph, 0, 0, 5, ok.data(), 0) == TD_OK);
    EXPECT(td_check_set(h, ph, 0, 4, 1, ok.data(), 0) == TD_OK);
    EXPECT(td_check_set(h, ph, 0, 0, 5, bad.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 0, 5, bad.data(), 1) == TD_OK);            // a device source is not read
    EXPECT(td_check_set(h, ph, 0, 0, 4, bad.data(), 0) == TD_OK);            // ... nor a host source past nb rows
    bad[0] = inf;
    EXPECT(td_check_set(h, ph, 0, 0, 1, bad.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 0, 5, nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, -1, 0, 5, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 3, 0, 5, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, -1, 2, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 0, 0, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 1, 5, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 0, 6, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_set(h, ph, 0, 2147483647, 2147483647, ok.data(), 0) == TD_EINVAL);      // (no overflow in the range test)
    EXPECT(td_check_set(h, ph, 1, 0, 5, ok.data(), 0) == TD_EINVAL);         // no touchdown constraint
    EXPECT(td_check_set(h, ph, 2, 0, 5, ok.data(), 0) == TD_ENOTSUP);        // not whole-body
    EXPECT(td_check_set(h32, ph, 0, 0, 5, ok.data(), 0) == TD_ENOTSUP);      // fp32 handle
    EXPECT(td_check_set(h, nullptr, 0, 0, 5, ok.data(), 0) == TD_EINVAL);
    EXPECT(td_check_range(h, ph, 0, 0, 5) == TD_OK && td_check_range(h, ph, 1, 0, 5) == TD_EINVAL && td_check_range(h, ph, 2, 0, 5) == TD_ENOTSUP);

    const int nx = 5, ny = 4, nm = 3;
    std::vector<double> H((size_t)nm * ny * nx);
    for (size_t i = 0; i < H.size(); i++) H[i] = 0.001 * (double)(i + 1);
    std::vector<int> map = {0, 1, 2, 1, 0}, mbad = {0, 1, 3, 1, 0};
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), map.data(), 0) == TD_OK);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_OK);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, nullptr, nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, nan, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, inf, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.0, 0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, -0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, nan, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, 0, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, 1025, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 1) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, 0, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, 4097, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 1) == TD_EINVAL);
    EXPECT(td_check_terrain(h, 1024, 1024, 5, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 1) == TD_EINVAL);      // more than 2^22 cells
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), mbad.data(), 0) == TD_EINVAL);
    EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), mbad.data(), 1) == TD_OK);          // a device map is not read
    { std::vector<double> Hn = H; Hn.back() = nan; EXPECT(td_check_terrain(h, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, Hn.data(), nullptr, 0) == TD_EINVAL); }
    EXPECT(td_check_terrain(h32, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0, H.data(), nullptr, 0) == TD_ENOTSUP);

    // lookups: phase 0 with per-problem rows (h = 2: three rows of 12 per problem), phase 1 shared (h = 1)
    const int B = 5;
    std::vector<double> fp0((size_t)B * 3 * 12, 7.0), fp1(2 * 12, 7.0);
    const double xs[6] = {-1.0, 0.2499999, -1e300, 1e300, nan, -0.76}, ys[6] = {-0.5, 1.4999999, 1e300, -1e300, 0.3, nan};
    for (int b = 0; b < B; b++) for (int l = 0; l < 4; l++) { double* p = &fp0[((size_t)b * 3 + 2) * 12 + 3 * l]; p[0] = xs[(b + l) % 6]; p[1] = ys[(b + 2 * l) % 6]; p[2] = nan; }
    for (int l = 0; l < 4; l++) { fp1[12 + 3 * l] = xs[l + 2]; fp1[12 + 3 * l + 1] = ys[l]; }
    const TdFootRef refs[2] = {{fp0.data(), 3, 2}, {fp1.data(), 0, 1}};
    const int on[2] = {1, 1}, off[2] = {1, 0};
    for (int use_map = 0; use_map < 2; use_map++) {
        const TdGrid g{H.data(), use_map ? map.data() : nullptr, 1, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.125};
        std::vector<double> out((size_t)2 * B * 4, -9.0);
        td_terrain_host(g, refs, on, 2, B, out.data());
        for (int pi = 0; pi < 2; pi++) for (int b = 0; b < B; b++) for (int l = 0; l < 4; l++) {
            const double v = out[((size_t)pi * B + b) * 4 + l], x = v - 0.125;
            const int m = use_map ? map[b] : 0;
            EXPECT(x >= H[(size_t)m * ny * nx] - 1e-12 && x <= H[(size_t)(m + 1) * ny * nx - 1] + 1e-12);      // a cell of the problem's own map
        }
        // corners and far points of problem 0 (map 0): x = -1 -> ix 0, y = -0.5 -> iy 0
        EXPECT(out[0] == 0.125 + H[0]);
        std::vector<double> o2((size_t)2 * B * 4, -9.0);
        td_terrain_host(g, refs, off, 2, B, o2.data());
        for (int i = 0; i < B * 4; i++) { EXPECT(o2[i] == out[i]); EXPECT(o2[(size_t)B * 4 + i] == -9.0); }      // a phase that is off is left alone
    }
    {   // strided map (an episode's [batch][n_samples] table read at sample 0) and the clamp of a map index outside the table
        std::vector<int> wide = {2, 9, 9, 1, 9, 9, 0, 9, 9, 7, 9, 9, -4, 9, 9};
        const TdGrid g{H.data(), wide.data(), 3, nx, ny, nm, -1.0, -0.5, 0.25, 0.5, 0.0};
        const int want[5] = {2, 1, 0, 2, 0};
        for (int b = 0; b < B; b++) {
            const double v = td_terrain_height(g, refs[1], b, 2);      // shared row: x = nan -> ix 0, y = ys[2] = 1e300 -> iy 3
            EXPECT(v == H[((size_t)want[b] * ny + 3) * nx + 0]);
        }
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
