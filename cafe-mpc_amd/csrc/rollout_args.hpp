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

// One argument record per kernel family: launch_rollout_list / launch_lq (hsddp_hip.hip) fill a record once, by name, and each launcher unpacks it into
// its kernel's positional list.  Members are named after the kernel parameters.  tdh (the window's touchdown heights [phase][batch][4],
// hsddp_touchdown.h), wtab (the cost-weight scales [batch][84], hsddp_weights.h) and ltab (the resolved constraint limits [phase][batch][12],
// hsddp_limits.h) are members of every record; only the _tdh / _pw / _lim kernels have the parameter, the others' launchers leave them where they are.
// RollCommon: what the three rollout families share (the terminal kernels take no slot_k, x0, fail and units)
struct RollCommon {
    const hs::PhaseDev* ph; int nph; const int *slot_phase, *slot_k; int nslots, batch; hs::ModelDev md; EpsList el; hs::OptDev opt; const double* x0; SlotArrays sa;
    const hs::ProbState* st; int mask; int* fail; unsigned long long* units; const int* plist; const double *tdh, *wtab, *ltab;
};
// the one-wave kernels: grid = candidates x problems x slots of the list; slot_list / nlist / unit_knots / nprob: rollout_body.hpp
struct RollArgs : RollCommon { const int* slot_list; int nlist, unit_knots, nprob; };
// the lane-quad running-knot kernels (hsddp_quad.hip): grid = one workgroup per unit (knot of the quad list x group of sixteen problems); nlist: problems in plist
struct QuadArgs : RollCommon { const int* qslots; int nq, nlist; };
// the lane-quad terminal-knot kernels (hsddp_quad.hip): one workgroup per unit (terminal slot of the list x group of sixteen problems)
struct QuadTermArgs : RollCommon { const int* tslots; int nlist; };
// the LQ kernels: grid = problems x slots (batch is k_lq_lim's, the row pitch of ltab)
struct LqArgs {
    const hs::PhaseDev* ph; int nph; const int *slot_phase, *slot_k; int nslots; hs::ModelDev md; hs::OptDev opt; const hs::ProbState* st; int mask, use_cache; unsigned long long* units;
    const double *wtab, *ltab; int batch;
};
// a record's members in the order of its family's kernel parameters (ROLL_ARGS, k_rollout_quad, k_rollout_quad_term, LQ_ARGS); a twin's launcher appends its tables
#define ROLL_FROM(a) a.ph, a.nph, a.slot_phase, a.slot_k, a.nslots, a.batch, a.md, a.el, a.opt, a.x0, a.sa, a.st, a.mask, a.fail, a.units, a.slot_list, a.nlist, a.unit_knots, a.plist, a.nprob
#define QUAD_FROM(a) a.ph, a.slot_phase, a.slot_k, a.qslots, a.nq, a.nslots, a.batch, a.md, a.el, a.opt, a.x0, a.sa, a.st, a.mask, a.fail, a.units, a.plist, a.nlist
#define QUAD_TERM_FROM(a) a.ph, a.nph, a.slot_phase, a.tslots, a.nslots, a.batch, a.md, a.el, a.opt, a.sa, a.st, a.mask, a.plist, a.nlist
#define LQ_FROM(a) a.ph, a.nph, a.slot_phase, a.slot_k, a.nslots, a.md, a.opt, a.st, a.mask, a.use_cache, a.units

void launch_k_rollout(unsigned grid, hipStream_t stream, const RollArgs& a);                    // hsddp_hip.hip
void launch_k_rollout_hkd(unsigned grid, hipStream_t stream, const RollArgs& a);
void launch_k_lq(unsigned grid, hipStream_t stream, const LqArgs& a);
void launch_k_lq_hkd(unsigned grid, hipStream_t stream, const LqArgs& a);
void launch_k_rollout_quad(unsigned grid, hipStream_t stream, const QuadArgs& a);               // hsddp_quad.hip
void launch_k_rollout_quad_term(unsigned grid, hipStream_t stream, const QuadTermArgs& a);
void launch_k_rollout_tdh(unsigned grid, hipStream_t stream, const RollArgs& a);                // hsddp_tdh.hip (hsddp_touchdown.h)
void launch_k_rollout_quad_term_tdh(unsigned grid, hipStream_t stream, const QuadTermArgs& a);
void launch_k_rollout_pw(unsigned grid, hipStream_t stream, const RollArgs& a);                 // hsddp_pw.hip (hsddp_weights.h)
void launch_k_rollout_quad_pw(unsigned grid, hipStream_t stream, const QuadArgs& a);
void launch_k_rollout_quad_term_pw(unsigned grid, hipStream_t stream, const QuadTermArgs& a);
void launch_k_lq_pw(unsigned grid, hipStream_t stream, const LqArgs& a);
void launch_k_rollout_lim(unsigned grid, hipStream_t stream, const RollArgs& a);                // hsddp_lim.hip (hsddp_limits.h)
void launch_k_rollout_quad_lim(unsigned grid, hipStream_t stream, const QuadArgs& a);
void launch_k_lq_lim(unsigned grid, hipStream_t stream, const LqArgs& a);

// the kernels that fill the tables: the heights from a terrain grid (hsddp_tdh.hip), the scales (hsddp_pw.hip), the limits and their mu column (hsddp_lim.hip)
namespace hs { struct TdGrid; struct WsPack; struct LimPack; struct LimMu; }
void launch_k_td_terrain(hipStream_t stream, const hs::PhaseDev* ph, int nph, int batch, const hs::TdGrid& g, double* out);
void launch_k_pack_weights(hipStream_t stream, const hs::WsPack& W);
void launch_k_pack_limits(hipStream_t stream, const hs::LimPack& W);
void launch_k_lim_mu(hipStream_t stream, const hs::LimMu& F);
