// TEST-ONLY: the closed-loop simulation program (cafe-mpc_amd/csrc/wb_sim.hpp) compiled for the HOST with -DHS_HOST_EMU, the four lanes of a
// quad evaluated together (QH of wb_quad.hpp), so that its logic - feedback product, step map, impact mode, divergence handling, layouts - is
// checked against the oracle where no GPU exists.  tests/test_sim_host.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hs_types.hpp"
#include "wb_sim.hpp"

using namespace hs;

extern "C" {
// One problem (b = 0), R samples.  Per phase p < nph: horizon[p], dt[p], bg_alpha[p], contact[4 p ..], td[4 p ..] and the policy Xbar[p] ((h+1) x 36),
// Ubar[p] (h x 12), K[p] (h x 432, column-major 12 x 36).  map: [3][n_steps] as hsddp_sim_create builds it.  Outputs as wbs_walk documents them.
int sim_emu_run(int nph, const int* horizon, const double* dt, const double* bg_alpha, const int* contact, const int* td, double* const* Xbar, double* const* Ubar,
                double* const* K, double psi_dyn, const int* map, int n_steps, int R, const double* x0, double* xfinal, double* rows, double* trajX, double* trajU) {
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p]; ph[p].dt = dt[p]; ph[p].bg_alpha = bg_alpha[p];
        for (int l = 0; l < 4; l++) { ph[p].contact[l] = contact[4 * p + l]; ph[p].td[l] = td[4 * p + l]; }
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < n_steps; s++) if (map[s] < 0 || map[s] >= nph || map[n_steps + s] < 0 || map[n_steps + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    for (int r = 0; r < R; r++) wbs_walk<QH>(ph.data(), md, map, n_steps, 0, (size_t)r, x0, xfinal, rows, trajX, trajU);
    return HSDDP_OK;
}
int sim_emu_row_doubles(void) { return SIM_ROW; }
}
