// The lane-quad rollout kernel of libhsddp_hip.so (wb_quad.hpp) and its launcher.  The Makefile compiles this file on its own with
// -mllvm -disable-machine-licm; hsddp_hip.hip includes it when it is built without -DHS_QUAD_SEPARATE (a one-command build of the library).
// Why the switch: the kernel evaluates the candidates of a probe launch in a LOOP around a knot program that fills the register file (256 VGPR +
// 256 AGPR at one wave per SIMD).  The machine-level invariant-code motion moves every constant the knot materialises (link inertias, polynomial
// coefficients, masks: a hundred registers' worth) in front of that loop, and the allocator then spills about 90 B per lane to scratch to carry them.
// Without that pass each trip forms its constants where it uses them, as the straight-line kernel always did: no scratch.  The switch holds
// for a whole compilation, and every other kernel of the library is to keep the code it has with the pass on - hence a compilation of its own.
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#include "wb_quad.hpp"
#include "wb_quad_term.hpp"
#include "rollout_args.hpp"

using namespace hs;

// The whole-body running knots of the phases with shooting nodes on LANE QUADS (wb_quad.hpp): one lane per leg, sixteen problems of the same
// knot per wave.  grid = knots of the list x ceil(problems / 16): ONE workgroup per unit, which evaluates the candidates el.e[0..n-1] of the launch
// one after the other (an ordinary or commit launch is the loop with n = 1); qslots: the slots this kernel owns.
// The candidates of a unit differ in eps only, so what they all read - Xbar / dX of knots k and k + 1, Ubar, dU, K dX and the reference row of
// the sixteen problems - is fetched from global memory ONCE, whole rows with the wave's lanes side by side, into LDS; the knot program then reads
// its inputs with ds_read instead of waiting for L2 in every candidate.  Row of a problem: QS_ROW doubles,
//   [0, 72) Xbar  [72, 144) dX  [144, 156) Ubar  [156, 168) dU  [168, 180) K dX  [180, 256) reference row (entries 76..79 are never read)
// QS_ROW = 268: 2 x 268 mod 64 = 24 dwords, the span of a quad's four leg-strided reads, so that the eight quads of a half wave fall on different
// banks both in the per-leg reads (stride 3 doubles) and in the replicated ones.  16 x 268 x 8 = 34 304 B (+ 256 B, QDL::lane_slot): four workgroups per CU, as many as
// one wave per SIMD can use.  Barrier parameters (eps / delta, up to 2 x 93 doubles per knot and problem) do not fit beside them and stay in global
// memory (the same CU re-reads them: L1 / L2 hits), as do the x0 rows (first knot of the horizon only).
#include "quad_term_body.hpp"      // QUAD_WPE, the QS_* row offsets, quad_term_body
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad(const PhaseDev* ph_, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch, ModelDev md, EpsList el, OptDev opt, const double* x0,
               SlotArrays sa, const ProbState* st, int mask, int* fail, unsigned long long* units, const int* plist, int nlist) {
#define QUAD_BODY_PW 0
#include "quad_body.hpp"      // the kernel's statements (shared with k_rollout_quad_pw, hsddp_pw.hip)
#undef QUAD_BODY_PW
}

void launch_k_rollout_quad(unsigned grid, hipStream_t stream, const QuadArgs& a) { hipLaunchKernelGGL(k_rollout_quad, dim3(grid), dim3(64), 0, stream, QUAD_FROM(a)); }

// The terminal knots the quad path owns (split_slots, hsddp_hip.hip: whole-body phase with shooting nodes whose successor, if any, is one too) on
// LANE QUADS: wbq_rollout_terminal (wb_quad_term.hpp).  Units, packing from plist and the candidate loop are k_rollout_quad's: grid = terminal slots of
// the list x ceil(problems / 16), one workgroup per unit, the candidates el.e[0..n-1] one after the other.  A kernel of its own and not a branch in
// k_rollout_quad: that kernel's register allocation (256 VGPR + AGPR at one wave per SIMD, nothing in scratch) is not to move, and a terminal unit
// has a tenth of the grid's units at the benchmark shape - it runs in the tail of the running knots' launch.
// Row of a problem, same offsets as above so that QuadIn serves both: [0, 36) Xbar[h]  [36, 72) Xbar[0] of the SUCCESSOR  [72, 108) dX[h]
// [108, 144) dX[0] of the successor  [180, 256) reference row of knot h.  Without a successor the phase itself stands in for it: valid addresses,
// values nobody reads.  Terminal knots are not counted in `units` (the one-wave program does not count them either).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QUAD_WPE, QUAD_WPE)))
k_rollout_quad_term(const PhaseDev* ph_, int nph, const int* slot_phase, const int* tslots, int nslots, int batch, ModelDev md, EpsList el, OptDev opt,
                    SlotArrays sa, const ProbState* st, int mask, const int* plist, int nlist) {
    __shared__ double stage[16 * QS_ROW];
    quad_term_body<false>(stage, ph_, nph, slot_phase, tslots, nslots, batch, md, el, opt, sa, st, mask, plist, nlist, nullptr);
}

void launch_k_rollout_quad_term(unsigned grid, hipStream_t stream, const QuadTermArgs& a) { hipLaunchKernelGGL(k_rollout_quad_term, dim3(grid), dim3(64), 0, stream, QUAD_TERM_FROM(a)); }

#ifdef QUAD_PROF
extern "C"
int hsddp_debug_quad_prof(unsigned long long* out24, int reset) {
    hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_quad_prof), 24 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[24] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_quad_prof), z, sizeof(z)); }
    return 0;
}
#endif
