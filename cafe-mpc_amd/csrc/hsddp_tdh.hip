// Per-problem touchdown heights (include/hsddp_touchdown.h): the rollout kernels that read them, the kernel that fills them from a terrain grid, and
// their launchers.  The Makefile compiles this file on its own (-DHS_TDH_SEPARATE for hsddp_hip.hip, with hsddp_quad.hip's QUAD_FLAGS because
// k_rollout_quad_term_tdh is that file's terminal kernel with one more operand); hsddp_hip.hip includes it when it is built without that switch (a
// one-command build of the library).  A translation unit of its own for the reason given in hsddp_sub.hip: the code objects of hsddp_hip.hip and
// hsddp_quad.hip keep every kernel where it is, and `make resources` lists the kernels it listed (`make resources-tdh` lists these).
//
//   k_rollout_tdh            rollout_body (rollout_body.hpp) with TDH on: the one-wave program - terminal knots in front of a projection or of a phase
//                            without shooting nodes and the chain behind them, single shooting (MS = 0), handles under HSDDP_QUAD_TERMINAL=0
//   k_rollout_quad_term_tdh  quad_term_body (quad_term_body.hpp) with TDH on: the terminal knots of the lane-quad path; lane = leg reads its own height
//   k_td_terrain             one lane per (phase, problem, leg): the height of the terrain at the phase's terminal reference foothold (touchdown.hpp)
// The heights are a kernel ARGUMENT, the window's table [phase][batch][4]: nothing is added to PhaseDev, whose layout every other kernel's scalar
// loads depend on.  Which launch runs them: roll_pick.hpp.
#ifdef HS_TDH_SEPARATE
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#include "rollout_body.hpp"
#include "quad_term_body.hpp"
#endif
#include "touchdown.hpp"

__global__ void __launch_bounds__(64) ROLL_ATTR k_rollout_tdh(ROLL_ARGS, const double* tdh) { __shared__ WbCore L; rollout_body<true, true>(L, ROLL_PASS, tdh); }

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad_term_tdh(const PhaseDev* ph_, int nph, const int* slot_phase, const int* tslots, int nslots, int batch, ModelDev md, EpsList el, OptDev opt,
                        SlotArrays sa, const ProbState* st, int mask, const int* plist, int nlist, const double* tdh) {
    __shared__ double stage[16 * QS_ROW];
    quad_term_body<true>(stage, ph_, nph, slot_phase, tslots, nslots, batch, md, el, opt, sa, st, mask, plist, nlist, tdh);
}

// grid = ceil(nph x batch x 4 / 256); lanes of phases that are not whole-body or have no touchdown constraint leave their entry alone
__global__ void __launch_bounds__(256) k_td_terrain(const PhaseDev* ph, int nph, int batch, hs::TdGrid g, double* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nph * batch * 4) return;
    const int leg = (int)(i & 3), b = (int)((i >> 2) % (size_t)batch), pi = (int)((i >> 2) / (size_t)batch);
    const PhaseDev& P = ph[pi];
    if (P.model != HSDDP_MODEL_WB || P.nt <= 0) return;
    const hs::TdFootRef r = {(const double*)P.foot_pos, P.ref_pb, P.h};
    out[i] = hs::td_terrain_height(g, r, b, leg);
}

void launch_k_rollout_tdh(unsigned grid, hipStream_t stream, const RollArgs& a) { hipLaunchKernelGGL(k_rollout_tdh, dim3(grid), dim3(64), 0, stream, ROLL_FROM(a), a.tdh); }
void launch_k_rollout_quad_term_tdh(unsigned grid, hipStream_t stream, const QuadTermArgs& a) { hipLaunchKernelGGL(k_rollout_quad_term_tdh, dim3(grid), dim3(64), 0, stream, QUAD_TERM_FROM(a), a.tdh); }
void launch_k_td_terrain(hipStream_t stream, const PhaseDev* ph, int nph, int batch, const hs::TdGrid& g, double* out) {
    const size_t n = (size_t)nph * batch * 4;
    hipLaunchKernelGGL(k_td_terrain, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ph, nph, batch, g, out);
}
