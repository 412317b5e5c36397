// TEST-ONLY: the two programs an MPC episode adds behind the walk (cafe-mpc_amd/csrc/episode.hpp) compiled for the HOST with -DHS_HOST_EMU: the
// commit with the 64 lanes of its wave one after the other (EpiWaveH), the pending reset map with the four lanes of a quad together (QH of
// wb_quad.hpp).  tests/test_episode_host.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hs_types.hpp"
#include "episode.hpp"

using namespace hs;

extern "C" {
int episode_emu_row_bytes(void) { return (int)sizeof(EpiRow); }

// The reset map of a whole-body phase (touchdown set td[4], Baumgarte alpha) on B states [B][36]; rows: [B] episode rows (a frozen problem is left
// alone); x0: [B][36] the hand-off destination.
int episode_emu_impact(const int* td, double bg_alpha, double psi_dyn, int B, const void* rows, double* state, double* x0) {
    PhaseDev P; std::memset(&P, 0, sizeof(P));
    P.model = HSDDP_MODEL_WB; P.n = 36; P.m = 12; P.p = 12; P.h = 1; P.bg_alpha = bg_alpha;
    for (int l = 0; l < 4; l++) P.td[l] = td[l];
    const ModelDev md = {std::cos(psi_dyn), std::sin(psi_dyn), -1.0, 0.0};
    for (int g = 0; g < B; g++) epi_impact<QH>(&P, md, 0, (size_t)g, (const EpiRow*)rows, state, x0);
    return HSDDP_OK;
}

// One commit over B problems.  Per phase p < nph: horizon[p], q[36 p ..], r[12 p ..], rref[p] (records of 80 doubles, (h+1) rows shared or
// B (h+1) rows per problem) and ref_pb[p] (0 or h+1).  status: [B] status of the last solve.  The other arguments are EpiCommitArgs' (null = absent).
int episode_emu_commit(int nph, const int* horizon, const double* q, const double* r, double* const* rref, const int* ref_pb, int B, const int* status,
                       int n_exec, int tick, int max_ticks, int handoff, const int* map, const double* simX, const double* simU, const double* simY,
                       const double* fin, const double* sim_rows, const double* extra, const double* grf_rows, void* rows, double* state, double* x0,
                       double* logX, double* logU, double* logY) {
    if (tick < 0 || tick >= max_ticks || n_exec <= 0) return HSDDP_EINVAL;
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p];
        for (int i = 0; i < 36; i++) ph[p].q[i] = q[36 * p + i];
        for (int j = 0; j < 12; j++) ph[p].r[j] = r[12 * p + j];
        ph[p].rref = rref[p]; ph[p].ref_pb = ref_pb[p];
    }
    for (int s = 0; s < n_exec; s++) if (map[s] < 0 || map[s] >= nph || map[n_exec + s] < 0 || map[n_exec + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    std::vector<ProbState> st(B);
    std::memset(st.data(), 0, sizeof(ProbState) * B);
    for (int b = 0; b < B; b++) st[b].status = status[b];
    EpiCommitArgs a;
    a.n_exec = n_exec; a.tick = tick; a.max_ticks = max_ticks; a.handoff = handoff; a.map = map; a.simX = simX; a.simU = simU; a.simY = simY;
    a.fin = fin; a.sim_rows = sim_rows; a.extra = extra; a.grf_rows = grf_rows; a.st = st.data(); a.rows = (EpiRow*)rows; a.state = state; a.x0 = x0;
    a.logX = logX; a.logU = logU; a.logY = logY;
    for (int b = 0; b < B; b++) epi_commit<EpiWaveH>(ph.data(), a, b);
    return HSDDP_OK;
}
}
