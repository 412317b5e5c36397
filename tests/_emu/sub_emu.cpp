// TEST-ONLY: the SUB-STEPPED closed-loop simulation program (cafe-mpc_amd/csrc/wb_sim.hpp with the SUB policies, include/hsddp_substep.h) compiled
// for the HOST with -DHS_HOST_EMU, the four lanes of a quad evaluated together (QH of wb_quad.hpp), as tests/_emu/sim_emu.cpp does for the plain
// program.  tests/test_substep_host.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
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
// One problem (b = 0 of the policy arrays, global index first_problem), R samples.  Policy, map and outputs as sim_emu_run takes them.
//   substeps >= 1: the SUB walk with that trip count (also for 1: the sub-stepped program, not the one the library launches for 1);
//   substeps == 0: the walk without the SUB switch, as sim_emu / mc_emu / grf_emu run it.
//   use_mc: the disturbed walk, arguments as mc_emu_run takes them (the generator compiled in iff a sigma is set); else seed .. extra are not read.
//   mu > 0: with contact-force records, arguments as grf_emu_run takes them; mu == 0: without, grf_rows and Y untouched.
int sub_emu_run(int nph, const int* horizon, const double* dt, const double* bg_alpha, const int* contact, const int* td, double* const* Xbar, double* const* Ubar,
                double* const* K, double psi_dyn, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU,
                int substeps, int use_mc, unsigned long long seed, int first_problem, const double* dist, int kick_step, const double* kick, double* extra,
                double mu, double fz_min, double* grf_rows, double* Y) {
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p]; ph[p].dt = dt[p]; ph[p].bg_alpha = bg_alpha[p];
        for (int l = 0; l < 4; l++) { ph[p].contact[l] = contact[4 * p + l]; ph[p].td[l] = td[4 * p + l]; }
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < n_steps; s++) if (map[s] < 0 || map[s] >= nph || map[n_steps + s] < 0 || map[n_steps + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    if (substeps < 0 || substeps > 64 || !(mu >= 0.0) || !(fz_min >= 0.0) || (mu > 0.0 && !grf_rows) || (use_mc && (!dist || !extra))) return HSDDP_EINVAL;
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    WbsMcArgs a; std::memset(&a, 0, sizeof(a));
    bool noise = false;
    if (use_mc) {
        a.seed = seed; a.first_problem = (unsigned long long)first_problem; a.su = dist[0]; a.sq = dist[1]; a.sv = dist[2]; a.umax = dist[3]; a.fall = dist[4];
        a.kick_step = kick ? kick_step : -1; a.R = R; a.kick = kick; a.extra = extra;
        noise = a.su > 0.0 || a.sq > 0.0 || a.sv > 0.0;
    }
    const WbsGrfArgs g = {mu, fz_min, grf_rows, Y};
    const WbsSubArgs sb = {substeps, 0};
    const bool grf = mu > 0.0;
#define RUN(...) walk_all(ph, md, map, n_steps, R, x0, xfinal, rows, trajX, trajU, __VA_ARGS__)
    if (substeps == 0) {
        if (!use_mc) { if (grf) RUN(WbsGrf{&g}); else RUN(WbsPlain{}); }
        else if (noise) { if (grf) RUN(WbsMcGrf<1>{&a, &g}); else RUN(WbsMc<1>{&a}); }
        else { if (grf) RUN(WbsMcGrf<0>{&a, &g}); else RUN(WbsMc<0>{&a}); }
    } else {
        if (!use_mc) { if (grf) RUN(WbsGrfSub{&g, &sb}); else RUN(WbsSub{&sb}); }
        else if (noise) { if (grf) RUN(WbsMcGrfSub<1>{&a, &g, &sb}); else RUN(WbsMcSub<1>{&a, &sb}); }
        else { if (grf) RUN(WbsMcGrfSub<0>{&a, &g, &sb}); else RUN(WbsMcSub<0>{&a, &sb}); }
    }
#undef RUN
    return HSDDP_OK;
}
// doubles of a lane's parked column: sub_emu_park_doubles(mc, grf) of the sub-stepped kernels
int sub_emu_park_doubles(int mc, int grf) { return (mc ? SIM_PARK_MC : SIM_PARK) + (grf ? SIM_GRF_PARK : 0) + SIM_SUB_PARK; }
}
