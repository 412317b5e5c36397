// TEST-ONLY: the closed-loop simulation program WITH TERRAIN AND EARLY SWING-FOOT TOUCHDOWN (cafe-mpc_amd/csrc/wb_sim.hpp with the TER policies,
// include/hsddp_terrain.h) compiled for the HOST with -DHS_HOST_EMU, the four lanes of a quad evaluated together (QH of wb_quad.hpp), as
// tests/_emu/uni_emu.cpp does for the program with unilateral contact alone.  On the host a quad is the whole wave.  tests/test_terrain_host.py builds
// it into a temporary directory, and tests/cpp/ter_walk_asan.cpp includes it into a stand-alone program; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hsddp_terrain.h"
#include "hs_types.hpp"
#include "wb_sim.hpp"

using namespace hs;

namespace {
template <class D>
void walk_all(std::vector<PhaseDev>& ph, const ModelDev& md, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU, const D& d) {
    for (int r = 0; r < R; r++) wbs_walk<QH, D>(ph.data(), md, map, n_steps, 0, (size_t)r, x0, xfinal, rows, trajX, trajU, nullptr, d);
}
}  // namespace

extern "C" {
// One problem, R samples; every argument up to hold as uni_emu_run takes it.  t, H: the terrain of include/hsddp_terrain.h; map_of: [R] or null (map 0);
// ter_rows: [R][SIM_TER_ROW]; E: [R][4] early flags, read at the head and written at the end under hold, or null (E starts empty).  The refusals are
// those of hsddp_terrain_set.
int ter_emu_run(int nph, const int* horizon, const double* dt, const double* bg_alpha, const int* contact, const int* td, double* const* Xbar, double* const* Ubar,
                double* const* K, double psi_dyn, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU,
                int substeps, int use_mc, unsigned long long seed, int first_problem, const double* dist, int kick_step, const double* kick, double* extra,
                double mu, double fz_min, double* grf_rows, double* Y, double fz_rel, double z_ground, double* uni_rows, double* F, const int* hold,
                const hsddp_terrain_t* t, const double* H, const int* map_of, double* ter_rows, double* E) {
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p]; ph[p].dt = dt[p]; ph[p].bg_alpha = bg_alpha[p];
        for (int l = 0; l < 4; l++) { ph[p].contact[l] = contact[4 * p + l]; ph[p].td[l] = td[4 * p + l]; }
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < n_steps; s++) if (map[s] < 0 || map[s] >= nph || map[n_steps + s] < 0 || map[n_steps + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    if (substeps < 1 || substeps > 64 || !(mu >= 0.0) || !(fz_min >= 0.0) || (mu > 0.0 && !grf_rows) || (use_mc && (!dist || !extra)) || !uni_rows || !ter_rows) return HSDDP_EINVAL;
    if (!std::isfinite(fz_rel) || !std::isfinite(z_ground) || !t || !H) return HSDDP_EINVAL;
    if (!std::isfinite(t->x0) || !std::isfinite(t->y0) || !std::isfinite(t->cx) || !std::isfinite(t->cy) || !std::isfinite(t->w_td) || !(t->cx > 0.0) || !(t->cy > 0.0) || t->w_td < 0.0) return HSDDP_EINVAL;
    if (t->nx < 1 || t->nx > 1024 || t->ny < 1 || t->ny > 1024 || t->n_maps < 1 || t->n_maps > 4096 || (size_t)t->n_maps * t->nx * t->ny > ((size_t)1 << 22)) return HSDDP_EINVAL;
    std::vector<int> maps((size_t)R, 0);
    for (int r = 0; r < R && map_of; r++) { if (map_of[r] < 0 || map_of[r] >= t->n_maps) return HSDDP_EINVAL; maps[r] = map_of[r]; }
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    WbsMcArgs a; std::memset(&a, 0, sizeof(a));
    bool noise = false;
    if (use_mc) {
        a.seed = seed; a.first_problem = (unsigned long long)first_problem; a.su = dist[0]; a.sq = dist[1]; a.sv = dist[2]; a.umax = dist[3]; a.fall = dist[4];
        a.kick_step = kick ? kick_step : -1; a.R = R; a.kick = kick; a.extra = extra;
        noise = a.su > 0.0 || a.sq > 0.0 || a.sv > 0.0;
    }
    std::vector<double> own((size_t)R * SIM_GRF_ROW);
    const WbsGrfArgs g = mu > 0.0 ? WbsGrfArgs{mu, fz_min, grf_rows, Y} : WbsGrfArgs{1.0, 0.0, own.data(), nullptr};
    const WbsSubArgs sb = {substeps, 0};
    const WbsUniArgs un = {fz_rel, z_ground, uni_rows, F, hold, 1, 0};
    const WbsTerArgs te = {H, maps.data(), t->nx, t->ny, t->n_maps, t->early ? 1 : 0, t->x0, t->y0, t->cx, t->cy, t->w_td, ter_rows, E};
#define RUN(...) walk_all(ph, md, map, n_steps, R, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (!use_mc) RUN(WbsTer{&g, &sb, &un, &te});
    else if (noise) RUN(WbsMcTer<1>{&a, &g, &sb, &un, &te});
    else RUN(WbsMcTer<0>{&a, &g, &sb, &un, &te});
#undef RUN
    return HSDDP_OK;
}
// doubles of a lane's parked column in the three kernels: ter_emu_park_doubles(mc)
int ter_emu_park_doubles(int mc) { return (mc ? SIM_PARK_MC : SIM_PARK) + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK; }
}
