// TEST-ONLY: the program a tick with policy latency runs in front of the walk (epi_latency of cafe-mpc_amd/csrc/episode.hpp, include/hsddp_latency.h)
// compiled for the HOST with -DHS_HOST_EMU: the 64 lanes of a wave one after the other (EpiWaveH), the (problem, step) pairs in the order of the
// kernel's grid.  tests/test_latency_host.py builds it into a temporary directory; never part of the product.
#define HS_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <vector>
#include "hsddp.h"
#include "hs_types.hpp"
#include "episode.hpp"

using namespace hs;

extern "C" {
int latency_emu_row_doubles(void) { return LAT_ROW; }

// One launch over B problems.  Per phase p < nph: horizon[p] and the handle's arrays Xbar[p] [B][h+1][36], Ubar[p] [B][h][12], K[p] [B][h][432].  map:
// [3][n_exec + D]; delay, n_stale, end_reason: [B]; prev, next: the stashes [B][D][516] (prev may be null when valid = 0 or D = 0); Xe, Ue, Ke: the
// effective rows in the DEVICE's layout, [n_exec][B][72 | 12 | 432].
int latency_emu_run(int nph, const int* horizon, double* const* Xbar, double* const* Ubar, double* const* K, int B, int n_exec, int D, int valid, const int* map,
                    const int* delay, int* n_stale, const int* end_reason, const double* prev, double* next, double* Xe, double* Ue, double* Ke) {
    if (n_exec <= 0 || D < 0 || D > n_exec || B <= 0) return HSDDP_EINVAL;
    const int L = n_exec + D;
    std::vector<PhaseDev> ph(nph);
    for (int p = 0; p < nph; p++) {
        std::memset(&ph[p], 0, sizeof(PhaseDev));
        ph[p].model = HSDDP_MODEL_WB; ph[p].n = 36; ph[p].m = 12; ph[p].p = 12; ph[p].h = horizon[p];
        ph[p].Xbar = Xbar[p]; ph[p].Ubar = Ubar[p]; ph[p].K = K[p];
    }
    for (int s = 0; s < L; s++) if (map[s] < 0 || map[s] >= nph || map[L + s] < 0 || map[L + s] >= horizon[map[s]]) return HSDDP_EINVAL;
    for (int b = 0; b < B; b++) if (delay[b] < 0 || delay[b] > D) return HSDDP_EINVAL;
    std::vector<EpiRow> rows(B);
    std::memset(rows.data(), 0, sizeof(EpiRow) * B);
    for (int b = 0; b < B; b++) rows[b].end_reason = end_reason[b];
    EpiLatArgs a;
    a.n_exec = n_exec; a.D = D; a.B = B; a.valid = valid; a.map = map; a.delay = delay; a.n_stale = n_stale; a.rows = rows.data();
    a.prev = prev; a.next = next; a.Xe = Xe; a.Ue = Ue; a.Ke = Ke;
    for (int r = 0; r < B * L; r++) epi_latency<EpiWaveH>(ph.data(), a, r / L, r % L);
    return HSDDP_OK;
}

// the rows of problems [b0, b0 + nb) out of the device's layout, as hsddp_latency_get_policy hands them out: Xo [nb][n_exec][72], Uo [nb][n_exec][12], Ko [nb][n_exec][432]
int latency_emu_get_policy(int B, int n_exec, int b0, int nb, const double* Xe, const double* Ue, const double* Ke, double* Xo, double* Uo, double* Ko) {
    if (b0 < 0 || nb <= 0 || b0 > B - nb) return HSDDP_EINVAL;
    const double* src[3] = {Xe, Ue, Ke}; double* dst[3] = {Xo, Uo, Ko}; const size_t w[3] = {72, 12, 432};
    for (int t = 0; t < 3; t++) for (size_t q = 0; q < (size_t)n_exec; q++) for (size_t i = 0; i < (size_t)nb; i++)
        std::memcpy(dst[t] + (i * n_exec + q) * w[t], src[t] + (q * B + b0 + i) * w[t], w[t] * 8);
    return HSDDP_OK;
}
}
