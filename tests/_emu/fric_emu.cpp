// TEST-ONLY: the closed-loop simulation program WITH COULOMB FRICTION (cafe-mpc_amd/csrc/wb_sim.hpp with the FRIC policies, include/hsddp_friction.h)
// compiled for the HOST with -DHS_HOST_EMU, the four lanes of a quad evaluated together (QH of wb_quad.hpp), as tests/_emu/ter_emu.cpp does for the
// program with terrain alone.  On the host a quad is the whole wave.  tests/fric_common.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hsddp_friction.h"
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
// One problem, R samples; every argument up to E as ter_emu_run takes it (t = null: the terrain is off - the one-cell flat map without early touchdown
// the library binds then).  f, mu: the friction parameters and table of include/hsddp_friction.h; mu_of: [R] or null (row 0); fric_rows: [R][SIM_FRIC_ROW];
// Sl, NF: [R][4] sliding flags and lagged normal forces, read at the head and written at the end under hold, or null (Sl starts empty).  The refusals
// are those of hsddp_terrain_set and hsddp_friction_set.
int fric_emu_run(int nph, const int* horizon, const double* dt, const double* bg_alpha, const int* contact, const int* td, double* const* Xbar, double* const* Ubar,
                 double* const* K, double psi_dyn, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU,
                 int substeps, int use_mc, unsigned long long seed, int first_problem, const double* dist, int kick_step, const double* kick, double* extra,
                 double mu_rec, double fz_min, double* grf_rows, double* Y, double fz_rel, double z_ground, double* uni_rows, double* F, const int* hold,
                 const hsddp_terrain_t* t, const double* H, const int* map_of, double* ter_rows, double* E,
                 const hsddp_friction_t* f, const double* mu, const int* mu_of, double* fric_rows, double* Sl, double* NF) {
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p]; ph[p].dt = dt[p]; ph[p].bg_alpha = bg_alpha[p];
        for (int l = 0; l < 4; l++) { ph[p].contact[l] = contact[4 * p + l]; ph[p].td[l] = td[4 * p + l]; }
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < n_steps; s++) if (map[s] < 0 || map[s] >= nph || map[n_steps + s] < 0 || map[n_steps + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    if (substeps < 1 || substeps > 64 || !(mu_rec >= 0.0) || !(fz_min >= 0.0) || (mu_rec > 0.0 && !grf_rows) || (use_mc && (!dist || !extra)) || !uni_rows || !fric_rows) return HSDDP_EINVAL;
    if (!std::isfinite(fz_rel) || !std::isfinite(z_ground)) return HSDDP_EINVAL;
    const hsddp_terrain_t flat = {1, 1, 1, 0, 0.0, 0.0, 1.0, 1.0, 0.0};
    const double flat_H = 0.0;
    std::vector<double> flat_rows((size_t)R * SIM_TER_ROW);
    if (!t) { t = &flat; H = &flat_H; map_of = nullptr; ter_rows = flat_rows.data(); E = nullptr; }
    else if (!H || !ter_rows) return HSDDP_EINVAL;
    if (!std::isfinite(t->x0) || !std::isfinite(t->y0) || !std::isfinite(t->cx) || !std::isfinite(t->cy) || !std::isfinite(t->w_td) || !(t->cx > 0.0) || !(t->cy > 0.0) || t->w_td < 0.0) return HSDDP_EINVAL;
    if (t->nx < 1 || t->nx > 1024 || t->ny < 1 || t->ny > 1024 || t->n_maps < 1 || t->n_maps > 4096 || (size_t)t->n_maps * t->nx * t->ny > ((size_t)1 << 22)) return HSDDP_EINVAL;
    std::vector<int> maps((size_t)R, 0), mus((size_t)R, 0);
    for (int r = 0; r < R && map_of; r++) { if (map_of[r] < 0 || map_of[r] >= t->n_maps) return HSDDP_EINVAL; maps[r] = map_of[r]; }
    if (!f || !mu || f->n_mu < 1 || f->n_mu > 65536 || !std::isfinite(f->v_stick) || f->v_stick < 0.0 || (Sl == nullptr) != (NF == nullptr)) return HSDDP_EINVAL;
    for (int i = 0; i < f->n_mu; i++) if (!std::isfinite(mu[2 * i]) || !std::isfinite(mu[2 * i + 1]) || mu[2 * i + 1] < 0.0 || mu[2 * i + 1] > mu[2 * i]) return HSDDP_EINVAL;
    for (int r = 0; r < R && mu_of; r++) { if (mu_of[r] < 0 || mu_of[r] >= f->n_mu) return HSDDP_EINVAL; mus[r] = mu_of[r]; }
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    WbsMcArgs a; std::memset(&a, 0, sizeof(a));
    bool noise = false;
    if (use_mc) {
        a.seed = seed; a.first_problem = (unsigned long long)first_problem; a.su = dist[0]; a.sq = dist[1]; a.sv = dist[2]; a.umax = dist[3]; a.fall = dist[4];
        a.kick_step = kick ? kick_step : -1; a.R = R; a.kick = kick; a.extra = extra;
        noise = a.su > 0.0 || a.sq > 0.0 || a.sv > 0.0;
    }
    std::vector<double> own((size_t)R * SIM_GRF_ROW);
    const WbsGrfArgs g = mu_rec > 0.0 ? WbsGrfArgs{mu_rec, fz_min, grf_rows, Y} : WbsGrfArgs{1.0, 0.0, own.data(), nullptr};
    const WbsSubArgs sb = {substeps, 0};
    const WbsUniArgs un = {fz_rel, z_ground, uni_rows, F, hold, 1, 0};
    const WbsTerArgs te = {H, maps.data(), t->nx, t->ny, t->n_maps, t->early ? 1 : 0, t->x0, t->y0, t->cx, t->cy, t->w_td, ter_rows, E};
    const WbsFricArgs fc = {mu, mus.data(), f->n_mu, 0, f->v_stick, fric_rows, Sl, NF};
#define RUN(...) walk_all(ph, md, map, n_steps, R, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (!use_mc) RUN(WbsFric{&g, &sb, &un, &te, &fc});
    else if (noise) RUN(WbsMcFric<1>{&a, &g, &sb, &un, &te, &fc});
    else RUN(WbsMcFric<0>{&a, &g, &sb, &un, &te, &fc});
#undef RUN
    return HSDDP_OK;
}
// doubles of a lane's parked column in the three kernels: fric_emu_park_doubles(mc)
int fric_emu_park_doubles(int mc) { return (mc ? SIM_PARK_MC : SIM_PARK) + SIM_GRF_PARK + SIM_SUB_PARK + SIM_UNI_PARK + SIM_TER_PARK + SIM_FRIC_PARK; }
}
