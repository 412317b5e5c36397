// Schedule-candidate ensembles (include/hsddp_ensemble.h): the winner rule and the two kernels above the solver.
//
//   ens_rank / ens_better  the selection rule of include/hsddp_ensemble.h as comparisons plus one division per threshold; compiled for the
//                          device here and for the host by the tests (ENS_RULE_ONLY: this section alone, no HIP headers), held bit for bit
//                          to the numpy statement ensemble.select_rows.
//   k_ens_select           one lane per problem: walks the S candidates' ProbState through a device table of pointers, writes the winner
//                          and the winner's hsddp_info_t row.
//   k_ens_pack             grid (n_steps, n rows): the MHPC_Command_lcmt words of (candidate, problem) pairs, each row bit-identical to what
//                          k_pack_command writes for that problem alone (same field order, same fp64 -> fp32 casts); the step -> (phase, k)
//                          map is the candidate's own (candidates may split their whole-body knots over phases differently).
#pragma once

#ifdef ENS_RULE_ONLY
#define ENS_HD inline
#else
#define ENS_HD __host__ __device__ inline
#endif

namespace hs {

struct EnsRank { double cost, viol; int tier; };

// tier and keys of one candidate's outcome (hsddp_info_t fields); td / tt / tp: dynamics_feas_thresh, tconstr_thresh, pconstr_thresh
ENS_HD EnsRank ens_rank(double cost, double dyn, double tc, double pc, int status, double td, double tt, double tp) {
    EnsRank r; r.cost = cost;
    double v = dyn / td, a = tc / tt;
    if (a > v) v = a;
    a = pc / tp;
    if (a > v) v = a;
    r.viol = v;
    const bool nan = cost != cost || dyn != dyn || tc != tc || pc != pc;
    r.tier = (nan || (status != 0 && status != 2)) ? 2 : (v <= 1.0 ? 0 : 1);
    return r;
}

// a strictly before b (a scan in candidate order that replaces only on `strictly before` gives ties to the lowest index)
ENS_HD bool ens_better(const EnsRank& a, const EnsRank& b) {
    if (a.tier != b.tier) return a.tier < b.tier;
    if (a.tier == 0) return a.cost < b.cost;
    if (a.tier == 1) return a.viol < b.viol || (a.viol == b.viol && a.cost < b.cost);
    return false;
}

}  // namespace hs

#ifndef ENS_RULE_ONLY
namespace hs {

constexpr int ENS_CMD_FIELDS = 15;
// MHPC_Command_lcmt per-step field widths (include/hsddp.h) and their prefix sums; a step has HSDDP_CMD_WORDS_PER_STEP = 1089 words
__constant__ int ens_cmd_off[ENS_CMD_FIELDS + 1] = {0, 1, 13, 16, 19, 31, 34, 37, 49, 61, 493, 505, 649, 1081, 1085, 1089};

__global__ void __launch_bounds__(256) k_ens_select(const ProbState* const* st, int S, int B, double td, double tt, double tp,
                                                    int* winner, hsddp_info_t* best) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int w = 0;
    EnsRank rb;
    for (int c = 0; c < S; c++) {
        const ProbState& s = st[c][b];
        const EnsRank r = ens_rank(s.actual_cost, s.feas, s.info_tconstr, s.info_pconstr, s.status, td, tt, tp);
        if (c == 0 || ens_better(r, rb)) { rb = r; w = c; }
    }
    winner[b] = w;
    if (best) {
        const ProbState& s = st[w][b];
        hsddp_info_t o;
        o.actual_cost = s.actual_cost; o.dyn_feas = s.feas; o.max_tconstr = s.info_tconstr; o.max_pconstr = s.info_pconstr;
        o.n_iters = s.iter; o.n_ls_iters = s.ls_total; o.n_reg_iters = s.reg_total; o.status = s.status;
        best[b] = o;
    }
}

// row i = pair (cand[i], prob[i]); step map of candidate c: map_phase / map_k [c * map_cap + s]; status: [S][st_stride] floats or nullptr
__global__ void __launch_bounds__(256) k_ens_pack(const PhaseDev* const* ph, const int* map_phase, const int* map_k, int map_cap,
                                                  const int* cand, const int* prob, int n_steps, double t0, double dt,
                                                  const float* status, int st_stride, unsigned int* out) {
    const int s = blockIdx.x, i = blockIdx.y;
    const int c = cand[i], b = prob[i];
    const int phase = map_phase[c * map_cap + s], k = map_k[c * map_cap + s];
    const PhaseDev& P = ph[c][phase];
    const double* X = P.Xbar + ((size_t)b * (P.h + 1) + k) * 36; const size_t kk = (size_t)b * P.h + k;
    const float* stc = status ? status + (size_t)c * st_stride + phase * 4 : nullptr;
    unsigned int* row = out + (size_t)i * (1 + (size_t)n_steps * HSDDP_CMD_WORDS_PER_STEP);
    if (s == 0 && threadIdx.x == 0) row[0] = (unsigned int)n_steps;
    for (int w = threadIdx.x; w < HSDDP_CMD_WORDS_PER_STEP; w += blockDim.x) {
        int f = 0;
        while (w >= ens_cmd_off[f + 1]) f++;
        const int e = w - ens_cmd_off[f];
        float v = 0.f; unsigned int word;
        switch (f) {
            case 0: v = (float)(t0 + s * dt); break;
            case 1: v = (float)P.Ubar[kk * 12 + e]; break;
            case 2: v = (float)X[3 + e]; break;
            case 3: v = (float)X[e]; break;
            case 4: v = (float)X[6 + e]; break;
            case 5: v = (float)X[18 + e]; break;
            case 6: v = (float)X[21 + e]; break;
            case 7: v = (float)X[24 + e]; break;
            case 8: v = (float)P.Y[kk * 12 + e]; break;
            case 9: v = (float)P.K[kk * 432 + e]; break;
            case 10: v = (float)P.Qu[kk * 12 + e]; break;
            case 11: v = (float)P.Quu[kk * 144 + e]; break;
            case 12: v = (float)P.Qux[kk * 432 + e]; break;
            case 13: break;
            default: v = stc ? stc[e] : 0.f; break;
        }
        word = f == 13 ? (unsigned int)P.contact[e] : __float_as_uint(v);
        const int wf = ens_cmd_off[f + 1] - ens_cmd_off[f];
        row[1 + (size_t)n_steps * ens_cmd_off[f] + (size_t)s * wf + e] = word;
    }
}

}  // namespace hs
#endif
