// What the rollout kernels of hsddp_hip.hip and the lane-quad rollout kernel share.  The quad kernel is a translation unit of its own
// (hsddp_quad.hip) because it is compiled with one more switch than the rest of the library (Makefile).
#pragma once
#include <hip/hip_runtime.h>
#include "hs_types.hpp"

struct SlotArrays { double *cost, *dsq, *ming, *maxh; };
enum { MASK_NONE = 0, MASK_LS = 1, MASK_INNER = 2, MASK_OUTER = 3, MASK_LS_OK = 4, MASK_COMMIT = 5 };
__device__ inline bool masked_out(const hs::ProbState& s, int mask) {
    if (mask == MASK_LS) return !s.ls_active;
    if (mask == MASK_INNER) return !s.inner_active;
    if (mask == MASK_OUTER) return !s.outer_active;
    if (mask == MASK_LS_OK) return !s.ls_success;
    if (mask == MASK_COMMIT) return !s.need_commit;
    return false;
}

// Step lengths of one launch.  Ordinary launches carry one (eps[0], or the problem's own ls_eps when from_state is set: the commit of a
// batched line search); a PROBE launch carries the candidates eps[0..n-1] of MultiPhaseDDP::line_search (MultiPhaseDDP.cpp:95-133) that
// are still to be tried (one-wave kernels: grid = candidates x problems x slots; quad kernel: a loop in each unit's wave), candidate c only leaves the per-slot partials of its merit function in
// slice c of the slot arrays - except candidate `writer` (the last of the search), which also writes the trajectories like an ordinary trial.
constexpr int MAXCAND = 12;
struct EpsList { double e[MAXCAND]; int n, writer, from_state; };

// k_rollout_quad (hsddp_quad.hip): grid = one workgroup per unit (knot of the quad list x group of sixteen problems)
void launch_k_rollout_quad(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch,
                           hs::ModelDev md, EpsList el, hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units,
                           const int* plist, int nlist);
// k_rollout_quad_term (hsddp_quad.hip): the terminal knots the quad path owns, one workgroup per unit (terminal slot of the list x group of sixteen problems)
void launch_k_rollout_quad_term(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* tslots, int nslots, int batch,
                                hs::ModelDev md, EpsList el, hs::OptDev opt, SlotArrays sa, const hs::ProbState* st, int mask, const int* plist, int nlist);

// The rollout kernels with per-problem touchdown heights and the kernel that fills the heights from a terrain grid (hsddp_tdh.hip, hsddp_touchdown.h);
// tdh: the window's table [phase][batch][4].  Arguments otherwise those of k_rollout / k_rollout_quad_term.
namespace hs { struct TdGrid; }
void launch_k_rollout_tdh(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* slot_k, int nslots, int batch, hs::ModelDev md, EpsList el,
                          hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units, const int* slot_list, int nlist,
                          int unit_knots, const int* plist, int nprob, const double* tdh);
void launch_k_rollout_quad_term_tdh(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* tslots, int nslots, int batch,
                                    hs::ModelDev md, EpsList el, hs::OptDev opt, SlotArrays sa, const hs::ProbState* st, int mask, const int* plist, int nlist, const double* tdh);
void launch_k_td_terrain(hipStream_t stream, const hs::PhaseDev* ph, int nph, int batch, const hs::TdGrid& g, double* out);

// The kernels with per-problem cost-weight scales and the kernel that writes their table (hsddp_pw.hip, hsddp_weights.h); wtab: the handle's table
// [batch][84].  Arguments otherwise those of k_rollout_tdh / k_rollout_quad / k_rollout_quad_term_tdh / k_lq.
namespace hs { struct WsPack; }
void launch_k_rollout_pw(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* slot_k, int nslots, int batch, hs::ModelDev md, EpsList el,
                         hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units, const int* slot_list, int nlist,
                         int unit_knots, const int* plist, int nprob, const double* tdh, const double* wtab);
void launch_k_rollout_quad_pw(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch,
                              hs::ModelDev md, EpsList el, hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units,
                              const int* plist, int nlist, const double* wtab);
void launch_k_rollout_quad_term_pw(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* tslots, int nslots, int batch,
                                   hs::ModelDev md, EpsList el, hs::OptDev opt, SlotArrays sa, const hs::ProbState* st, int mask, const int* plist, int nlist, const double* tdh,
                                   const double* wtab);
void launch_k_lq_pw(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* slot_k, int nslots, hs::ModelDev md, hs::OptDev opt,
                    const hs::ProbState* st, int mask, int use_cache, unsigned long long* units, const double* wtab);
void launch_k_pack_weights(hipStream_t stream, const hs::WsPack& W);

// The kernels with per-problem constraint limits and the kernels that write their tables (hsddp_lim.hip, hsddp_limits.h); ltab: the handle's resolved
// table [phase][batch][12].  Arguments otherwise those of k_rollout_pw / k_rollout_quad_pw / k_lq_pw.
namespace hs { struct LimPack; struct LimMu; }
void launch_k_rollout_lim(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* slot_k, int nslots, int batch, hs::ModelDev md, EpsList el,
                          hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units, const int* slot_list, int nlist,
                          int unit_knots, const int* plist, int nprob, const double* tdh, const double* wtab, const double* ltab);
void launch_k_rollout_quad_lim(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch,
                               hs::ModelDev md, EpsList el, hs::OptDev opt, const double* x0, SlotArrays sa, const hs::ProbState* st, int mask, int* fail, unsigned long long* units,
                               const int* plist, int nlist, const double* wtab, const double* ltab);
void launch_k_lq_lim(unsigned grid, hipStream_t stream, const hs::PhaseDev* ph, int nph, const int* slot_phase, const int* slot_k, int nslots, hs::ModelDev md, hs::OptDev opt,
                     const hs::ProbState* st, int mask, int use_cache, unsigned long long* units, const double* wtab, const double* ltab, int batch);
void launch_k_pack_limits(hipStream_t stream, const hs::LimPack& W);
void launch_k_lim_mu(hipStream_t stream, const hs::LimMu& F);
