// Per-problem cost-weight scales (include/hsddp_weights.h): the kernels that read them, the kernel that writes their table, and the launchers.  The
// Makefile compiles this file on its own (-DHS_PW_SEPARATE for hsddp_hip.hip, with hsddp_quad.hip's QUAD_FLAGS because two of its kernels are that
// file's with one more operand); hsddp_hip.hip includes it when it is built without that switch (a one-command build of the library).  A translation
// unit of its own for the reason given in hsddp_sub.hip: the code objects of every other file keep every kernel where it is, and `make resources`
// lists the kernels it listed (`make resources-pw` lists these).
//
//   k_rollout_pw             rollout_body (rollout_body.hpp) with PW and TDH on: the one-wave program, what k_rollout / k_rollout_tdh run
//   k_rollout_quad_pw        the statements of k_rollout_quad (quad_body.hpp) with QUAD_BODY_PW: the whole-body running knots on lane quads
//   k_rollout_quad_term_pw   quad_term_body (quad_term_body.hpp) with PW and TDH on: the terminal knots of the lane-quad path
//   k_lq_pw                  lq_body (lq_body.hpp) with PW on
//   k_pack_weights           one launch per hsddp_weights_set: the rows it writes (weights.hpp)
// The table is a kernel ARGUMENT, [batch][84] = sq[36] | sr[12] | sqf[36] per problem: nothing is added to PhaseDev.  The two kernels that hold
// terminal programs are instantiated with the touchdown heights of hsddp_touchdown.h compiled in, so scales and heights combine without a third and
// fourth pair of kernels: a window without heights of its own hands them a table that holds each phase's ground_height (weights_host.hpp).
// Which launch runs them, and that the heights table must be ready first: roll_pick.hpp.
#ifdef HS_PW_SEPARATE
#include <hip/hip_runtime.h>
#include <algorithm>
#include "hs_types.hpp"
#include "rollout_body.hpp"
#include "quad_term_body.hpp"
#endif
#include "lq_body.hpp"
#include "weights.hpp"

__global__ void __launch_bounds__(64) ROLL_ATTR k_rollout_pw(ROLL_ARGS, const double* tdh, const double* wtab) { __shared__ WbCore L; rollout_body<true, true, true>(L, ROLL_PASS, tdh, wtab); }

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad_pw(const PhaseDev* ph_, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch, ModelDev md, EpsList el, OptDev opt, const double* x0,
                  SlotArrays sa, const ProbState* st, int mask, int* fail, unsigned long long* units, const int* plist, int nlist, const double* wtab) {
#define QUAD_BODY_PW 1
#include "quad_body.hpp"      // k_rollout_quad's statements, the knot with the scales
#undef QUAD_BODY_PW
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad_term_pw(const PhaseDev* ph_, int nph, const int* slot_phase, const int* tslots, int nslots, int batch, ModelDev md, EpsList el, OptDev opt,
                       SlotArrays sa, const ProbState* st, int mask, const int* plist, int nlist, const double* tdh, const double* wtab) {
    __shared__ double stage[16 * QS_ROW];
    quad_term_body<true, true>(stage, ph_, nph, slot_phase, tslots, nslots, batch, md, el, opt, sa, st, mask, plist, nlist, tdh, wtab);
}

__global__ void __launch_bounds__(LQ_NT) LQ_ATTR k_lq_pw(LQ_ARGS, const double* wtab) { __shared__ WbLqLds L; lq_body<true, LQ_NT, true>(L, LQ_PASS, wtab); }

__global__ void __launch_bounds__(256) k_pack_weights(hs::WsPack W) {
    const size_t n = hs::ws_count(W), o = (size_t)W.p0 * hs::WSP_ROW;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) W.dst[o + i] = hs::ws_value(W, i);
}

void launch_k_rollout_pw(unsigned grid, hipStream_t stream, const RollArgs& a) { hipLaunchKernelGGL(k_rollout_pw, dim3(grid), dim3(64), 0, stream, ROLL_FROM(a), a.tdh, a.wtab); }
void launch_k_rollout_quad_pw(unsigned grid, hipStream_t stream, const QuadArgs& a) { hipLaunchKernelGGL(k_rollout_quad_pw, dim3(grid), dim3(64), 0, stream, QUAD_FROM(a), a.wtab); }
void launch_k_rollout_quad_term_pw(unsigned grid, hipStream_t stream, const QuadTermArgs& a) { hipLaunchKernelGGL(k_rollout_quad_term_pw, dim3(grid), dim3(64), 0, stream, QUAD_TERM_FROM(a), a.tdh, a.wtab); }
void launch_k_lq_pw(unsigned grid, hipStream_t stream, const LqArgs& a) { hipLaunchKernelGGL(k_lq_pw, dim3(grid), dim3(LQ_NT), 0, stream, LQ_FROM(a), a.wtab); }
void launch_k_pack_weights(hipStream_t stream, const hs::WsPack& W) {
    const size_t n = hs::ws_count(W);
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_pack_weights, dim3(grid), dim3(256), 0, stream, W);
}
