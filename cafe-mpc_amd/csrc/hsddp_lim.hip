// Per-problem constraint limits (include/hsddp_limits.h): the kernels that read them, the kernels that write their tables, and the launchers.  The
// Makefile compiles this file on its own (-DHS_LIM_SEPARATE for hsddp_hip.hip, with hsddp_quad.hip's QUAD_FLAGS because one of its kernels is that
// file's with two more operands); hsddp_hip.hip includes it when it is built without that switch and without -DHS_PW_SEPARATE (a one-command build of
// the library).  A translation unit of its own for the reason given in hsddp_sub.hip: the code objects of every other file keep every kernel where
// it is, and `make resources` lists the kernels it listed (`make resources-lim` lists these).
//
//   k_rollout_lim        rollout_body (rollout_body.hpp) with PW, TDH and LIM on: the one-wave program, what k_rollout / k_rollout_pw run
//   k_rollout_quad_lim   the statements of k_rollout_quad (quad_body.hpp) with QUAD_BODY_PW and QUAD_BODY_LIM: the whole-body running knots on lane quads
//   k_lq_lim             lq_body (lq_body.hpp) with PW and LIM on
//   k_pack_limits        one launch per hsddp_limits_set and per hsddp_reconfigure while a table is set: user rows and resolved rows (limits.hpp)
//   k_lim_mu             one launch per hsddp_episode_plan_friction: the mu column from the episode's friction table (limits.hpp; the name says "mu"
//                        because tests/test_friction_host.py lets no kernel of libhsddp_hip.so carry the friction walks' tag in its name)
// The resolved table is a kernel ARGUMENT, [phase][batch][12]: nothing is added to PhaseDev, and the knots test nothing - every entry is the value to
// use.  Terminal knots read no path-constraint limit: on lane quads they go on running k_rollout_quad_term / _tdh / _pw.  The kernels here have the
// scales of hsddp_weights.h compiled in; a handle with limits and no scales hands them a table of 1.0 (limits_host.hpp).  Which launch runs
// which of them, and with which scale table: roll_pick.hpp.
#ifdef HS_LIM_SEPARATE
#include <hip/hip_runtime.h>
#include <algorithm>
#include "hs_types.hpp"
#include "rollout_body.hpp"
#include "quad_term_body.hpp"
#endif
#include "lq_body.hpp"
#include "limits.hpp"

__global__ void __launch_bounds__(64) ROLL_ATTR k_rollout_lim(ROLL_ARGS, const double* tdh, const double* wtab, const double* ltab) {
    __shared__ WbCore L; rollout_body<true, true, true, true>(L, ROLL_PASS, tdh, wtab, ltab);
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad_lim(const PhaseDev* ph_, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch, ModelDev md, EpsList el, OptDev opt, const double* x0,
                   SlotArrays sa, const ProbState* st, int mask, int* fail, unsigned long long* units, const int* plist, int nlist, const double* wtab, const double* ltab) {
#define QUAD_BODY_PW 1
#define QUAD_BODY_LIM 1
#include "quad_body.hpp"      // k_rollout_quad's statements, the knot with the scales and the limits
#undef QUAD_BODY_LIM
#undef QUAD_BODY_PW
}

__global__ void __launch_bounds__(LQ_NT) LQ_ATTR k_lq_lim(LQ_ARGS, const double* wtab, const double* ltab, int batch) {
    __shared__ WbLqLds L; lq_body<true, LQ_NT, true, true>(L, LQ_PASS, wtab, ltab, batch);
}

__global__ void __launch_bounds__(256) k_pack_limits(hs::LimPack W) {
    const size_t n = hs::lim_pack_count(W);
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) hs::lim_pack_item(W, i);
}

__global__ void __launch_bounds__(256) k_lim_mu(hs::LimMu F) {
    for (size_t b = (size_t)blockIdx.x * 256u + threadIdx.x; b < (size_t)F.batch; b += (size_t)gridDim.x * 256u) hs::lim_mu_item(F, (int)b);
}

void launch_k_rollout_lim(unsigned grid, hipStream_t stream, const RollArgs& a) { hipLaunchKernelGGL(k_rollout_lim, dim3(grid), dim3(64), 0, stream, ROLL_FROM(a), a.tdh, a.wtab, a.ltab); }
void launch_k_rollout_quad_lim(unsigned grid, hipStream_t stream, const QuadArgs& a) { hipLaunchKernelGGL(k_rollout_quad_lim, dim3(grid), dim3(64), 0, stream, QUAD_FROM(a), a.wtab, a.ltab); }
void launch_k_lq_lim(unsigned grid, hipStream_t stream, const LqArgs& a) { hipLaunchKernelGGL(k_lq_lim, dim3(grid), dim3(LQ_NT), 0, stream, LQ_FROM(a), a.wtab, a.ltab, a.batch); }
void launch_k_pack_limits(hipStream_t stream, const hs::LimPack& W) {
    const size_t n = hs::lim_pack_count(W);
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_pack_limits, dim3(grid), dim3(256), 0, stream, W);
}
void launch_k_lim_mu(hipStream_t stream, const hs::LimMu& F) {
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)F.batch + 255) / 256, 4096);
    hipLaunchKernelGGL(k_lim_mu, dim3(grid), dim3(256), 0, stream, F);
}
