// TEST-ONLY: a stand-alone program around the host build of the walk with terrain and early touchdown (tests/_emu/ter_emu.cpp, included below), which
// tests/test_terrain_host.py compiles with -fsanitize=address,undefined and runs as a program.  The only data-dependent address of the feature is the
// grid index, so the walk is run where that index is pushed hardest: on the "edge" case of tests/ter_common.py (every foot outside a 4 x 4 grid), and on
// that case with a base position of 1e300 and of NaN.
//
//   ter_walk_asan FILE      FILE: doubles, written by the test -
//     nph n_steps R S psi_dyn | per phase: horizon dt bg_alpha contact[4] td[4] | per phase: Xbar [(h+1) 36], Ubar [h 12], K [h 432] | map [3 n_steps] |
//     x0 [R 36] | kick_step kick [R 36] | dist [5] seed | fz_rel z_ground | nx ny n_maps early x0 y0 cx cy w_td | H [n_maps ny nx] | map_of [R]
#include <cstdio>
#include <cstdlib>
#include "../_emu/ter_emu.cpp"

namespace {
struct Reader {
    std::vector<double> d; size_t at = 0;
    double one() { if (at >= d.size()) { std::fprintf(stderr, "ter_walk_asan: input too short\n"); std::exit(2); } return d[at++]; }
    int num() { return (int)one(); }
    std::vector<double> block(size_t n) { std::vector<double> o(n); for (auto& v : o) v = one(); return o; }
    std::vector<int> ints(size_t n) { std::vector<int> o(n); for (auto& v : o) v = num(); return o; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: ter_walk_asan FILE\n"); return 2; }
    Reader in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        double buf[4096]; size_t n;
        while ((n = std::fread(buf, sizeof(double), 4096, f)) > 0) in.d.insert(in.d.end(), buf, buf + n);
        std::fclose(f);
    }
    const int nph = in.num(), n_steps = in.num(), R = in.num(), S = in.num();
    const double psi_dyn = in.one();
    std::vector<int> horizon(nph), contact(4 * nph), td(4 * nph); std::vector<double> dt(nph), alpha(nph);
    for (int p = 0; p < nph; p++) {
        horizon[p] = in.num(); dt[p] = in.one(); alpha[p] = in.one();
        for (int l = 0; l < 4; l++) contact[4 * p + l] = in.num();
        for (int l = 0; l < 4; l++) td[4 * p + l] = in.num();
    }
    std::vector<std::vector<double>> Xb(nph), Ub(nph), Kb(nph); std::vector<double*> xp(nph), up(nph), kp(nph);
    for (int p = 0; p < nph; p++) {
        Xb[p] = in.block((size_t)(horizon[p] + 1) * 36); Ub[p] = in.block((size_t)horizon[p] * 12); Kb[p] = in.block((size_t)horizon[p] * 432);
        xp[p] = Xb[p].data(); up[p] = Ub[p].data(); kp[p] = Kb[p].data();
    }
    const std::vector<int> map = in.ints((size_t)3 * n_steps);
    const std::vector<double> x0 = in.block((size_t)R * 36);
    const int kick_step = in.num();
    const std::vector<double> kick = in.block((size_t)R * 36), dist = in.block(5);
    const unsigned long long seed = (unsigned long long)in.one();
    const double fz_rel = in.one(), z_ground = in.one();
    hsddp_terrain_t t;
    t.nx = in.num(); t.ny = in.num(); t.n_maps = in.num(); t.early = in.num(); t.x0 = in.one(); t.y0 = in.one(); t.cx = in.one(); t.cy = in.one(); t.w_td = in.one();
    const std::vector<double> H = in.block((size_t)t.n_maps * t.ny * t.nx);      // (exactly the grid: a read past it is a heap overflow the sanitizer reports)
    const std::vector<int> map_of = in.ints((size_t)R);
    const char* names[3] = {"edge case", "base position 1e300", "base position NaN"};
    for (int v = 0; v < 3; v++) {
        std::vector<double> x = x0;
        if (v > 0) for (int r = 0; r < R; r++) for (int i = 0; i < 3; i++) x[(size_t)r * 36 + i] = v == 1 ? (i == 1 ? -1e300 : 1e300) : std::nan("");
        std::vector<double> xf((size_t)R * 36), rows((size_t)R * SIM_ROW), X((size_t)R * (n_steps + 1) * 36), U((size_t)R * n_steps * 12), extra((size_t)R * 2),
            g((size_t)R * SIM_GRF_ROW), Y((size_t)R * n_steps * 12), c((size_t)R * SIM_UNI_ROW), tr((size_t)R * SIM_TER_ROW), F((size_t)R * 4, 0.0), E((size_t)R * 4, 0.0);
        const int rc = ter_emu_run(nph, horizon.data(), dt.data(), alpha.data(), contact.data(), td.data(), xp.data(), up.data(), kp.data(), psi_dyn,
                                   map.data(), n_steps, R, x.data(), xf.data(), rows.data(), X.data(), U.data(), S, 1, seed, 0, dist.data(), kick_step, kick.data(), extra.data(),
                                   0.6, 0.0, g.data(), Y.data(), fz_rel, z_ground, c.data(), F.data(), nullptr, &t, H.data(), map_of.data(), tr.data(), E.data());
        if (rc != 0) { std::fprintf(stderr, "ter_walk_asan: %s: rc %d\n", names[v], rc); return 1; }
        double early = 0.0, bad = 0.0;
        for (int r = 0; r < R; r++) { early += tr[(size_t)r * SIM_TER_ROW + 1]; bad += rows[(size_t)r * SIM_ROW + 4] >= 0.0 ? 1.0 : 0.0; }
        std::printf("ter_walk_asan: %s: early touchdowns %.0f, diverged samples %.0f of %d\n", names[v], early, bad, R);
    }
    std::printf("ter_walk_asan: clean\n");
    return 0;
}
