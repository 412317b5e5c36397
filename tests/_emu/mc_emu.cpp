// TEST-ONLY: the DISTURBED closed-loop simulation program (cafe-mpc_amd/csrc/wb_sim.hpp with the WbsMc policy, include/hsddp_mc.h) compiled for
// the HOST with -DHS_HOST_EMU, the four lanes of a quad evaluated together (QH of wb_quad.hpp), as tests/_emu/sim_emu.cpp does for the plain
// program.  tests/test_mc_host.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hs_types.hpp"
#include "wb_sim.hpp"

using namespace hs;

extern "C" {
// One problem (b = 0 of the policy arrays, global index first_problem), R samples.  Policy and map as sim_emu_run takes them; dist: seed given apart,
// then sigma_u, sigma_q, sigma_v, u_max, fall_height; kick: [R][36] or null; extra: [R][2] first_fall | n_sat.
int mc_emu_run(int nph, const int* horizon, const double* dt, const double* bg_alpha, const int* contact, const int* td, double* const* Xbar, double* const* Ubar,
               double* const* K, double psi_dyn, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU,
               unsigned long long seed, int first_problem, const double* dist, int kick_step, const double* kick, double* extra) {
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p]; ph[p].dt = dt[p]; ph[p].bg_alpha = bg_alpha[p];
        for (int l = 0; l < 4; l++) { ph[p].contact[l] = contact[4 * p + l]; ph[p].td[l] = td[4 * p + l]; }
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < n_steps; s++) if (map[s] < 0 || map[s] >= nph || map[n_steps + s] < 0 || map[n_steps + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    WbsMcArgs a;
    a.seed = seed; a.first_problem = (unsigned long long)first_problem; a.su = dist[0]; a.sq = dist[1]; a.sv = dist[2]; a.umax = dist[3]; a.fall = dist[4];
    a.kick_step = kick ? kick_step : -1; a.R = R; a.kick = kick; a.extra = extra;
    // as hsddp_mc_run picks the kernel: the walk without the generator when no sigma is set
    if (a.su > 0.0 || a.sq > 0.0 || a.sv > 0.0) { for (int r = 0; r < R; r++) wbs_walk<QH, WbsMc<1>>(ph.data(), md, map, n_steps, 0, (size_t)r, x0, xfinal, rows, trajX, trajU, nullptr, WbsMc<1>{&a}); }
    else { for (int r = 0; r < R; r++) wbs_walk<QH, WbsMc<0>>(ph.data(), md, map, n_steps, 0, (size_t)r, x0, xfinal, rows, trajX, trajU, nullptr, WbsMc<0>{&a}); }
    return HSDDP_OK;
}
double mc_emu_draw(unsigned long long seed, unsigned long long n) { return wbs_mc_draw(seed, n); }
int mc_emu_park_doubles(void) { return SIM_PARK_MC; }
}
