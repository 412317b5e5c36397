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
    PhaseC* ph = (PhaseC*)ph_;
    __shared__ double stage[16 * QS_ROW];
    // plist / nlist: the problems this launch is for (null: all of the batch, `mask` picks).  A probe launch of a line search or a commit launch only
    // concerns some problems; packed sixteen to a wave from the list the deciding kernel left behind, its waves are full whatever the share is
    const int nprob = plist != nullptr ? nlist : batch;
    const int nbg = (nprob + 15) >> 4;
    const int qi = blockIdx.x / nbg, bg = blockIdx.x - qi * nbg;
    const int s = qslots[qi], pi = slot_phase[s], k = slot_k[s];
    PhaseC& P = ph[pi];
    const int t = threadIdx.x;
    const int ix = bg * 16 + (t >> 2);
    const int b = ix < nprob ? (plist != nullptr ? plist[ix] : ix) : batch;
    const bool active = b < batch && !masked_out(st[b < batch ? b : 0], mask);
    {   // knots this launch rolls out (measurement only): one atomic per wave, every candidate of the loop counted
        const unsigned long long m = __ballot(active && (t & 3) == 0);
        if (m == 0) return;      // none of the wave's problems takes part in this launch (a masked launch over the whole batch): nothing to stage
        if (t == 0) atomicAdd(units, (unsigned long long)(__popcll(m) * el.n));
    }
    {   // stage the rows of the wave's sixteen problems: per problem three whole-wave loads (Xbar, dX, reference row: entries 0..63) and one that
        // gathers the six tails; all of them issued before the first is written to LDS.  A group that is only partly filled (nprob no multiple of 16)
        // stages its last problem again in the empty places, so nothing is read beyond the list or the batch.
        const int h = P.h;
        const HS_GLOBAL double *pX = P.Xbar, *pdX = P.dX, *pU = P.Ubar, *pdU = P.dU, *pKdX = P.KdX, *pR = P.rref;
        const int seg = t < 8 ? 0 : t < 16 ? 1 : t < 28 ? 2 : t < 40 ? 3 : t < 52 ? 4 : 5;      // tail of Xbar, dX (entries 64..71), Ubar, dU, K dX, reference row (64..75)
        const int toff = seg == 0 ? 64 + t : seg == 1 ? 64 + (t - 8) : seg == 2 ? t - 16 : seg == 3 ? t - 28 : seg == 4 ? t - 40 : 64 + (t - 52);      // entry within its array's row
        const int tdst = seg == 0 ? toff : seg == 1 ? QS_DX + toff : seg == 2 ? QS_U + toff : seg == 3 ? QS_DU + toff : seg == 4 ? QS_KDX + toff : QS_RR + toff;
        // the tails' source as ONE address form for every lane, base + (problem x rows-per-problem + knot's row + entry): the lane's array is picked here, once
        const HS_GLOBAL double* tsrc = seg == 0 ? pX : seg == 1 ? pdX : seg == 2 ? pU : seg == 3 ? pdU : seg == 4 ? pKdX : pR;
        const unsigned tmul = seg < 2 ? (unsigned)(h + 1) * 36u : seg < 5 ? (unsigned)h * 12u : (unsigned)P.ref_pb * 80u;
        const size_t tadd = (size_t)k * (seg < 2 ? 36 : seg < 5 ? 12 : 80) + toff;
        const int ixl = min(bg * 16 + (t & 15), nprob - 1);
        const int bl = plist != nullptr ? plist[ixl] : ixl;      // lane p (mod 16) holds problem p of the group
        double v[16][4];
        _Pragma("unroll")
        for (int p = 0; p < 16; p++) {
            const int bp = __builtin_amdgcn_readlane(bl, p);
            const size_t kx = ((size_t)bp * (h + 1) + k) * 36, kr = ref_row(P, bp, k) * 80;
            v[p][0] = pX[kx + t]; v[p][1] = pdX[kx + t]; v[p][2] = pR[kr + t]; v[p][3] = tsrc[(size_t)bp * tmul + tadd];
        }
        _Pragma("unroll")
        for (int p = 0; p < 16; p++) {
            double* row = stage + p * QS_ROW;
            row[t] = v[p][0]; row[QS_DX + t] = v[p][1]; row[QS_RR + t] = v[p][2]; row[tdst] = v[p][3];
        }
    }
    QDL::lane_slot()[t] = t & 3;
    __syncthreads();      // (one wave: orders the LDS writes above before the other lanes' reads below)
    if (!active) return;      // (a quad leaves or stays as a whole: the cross-lane steps below need all four lanes)
    _Pragma("nounroll")
    for (int c = 0; c < el.n; c++) {      // el.writer is the last candidate of a launch or none: `wr` is uniform over the wave in every trip
        // Every trip starts from a descriptor pointer, a problem, a knot and a row offset the compiler cannot see through: nothing a trip reads
        // or derives from them (its LDS rows, the descriptor's scalars, addresses) may be hoisted out of the loop and held in registers across
        // it - the knot's live set has no room for that (QDL, wb_quad.hpp, does the same for what depends on the lane).
        PhaseC* Pc = &P; HS_PIN_S(Pc);
        int bc = b, kc = k; HS_PIN_S(kc);
        int ro = (t >> 2) * QS_ROW; HS_PIN(bc); HS_PIN(ro);
        const HS_LDS double* row = (const HS_LDS double*)stage + ro;
        const QuadIn<const HS_LDS double*> in = {row, row + QS_DX, row + QS_U, row + QS_DU, row + QS_KDX, row + QS_RR};
        const double eps = el.from_state ? st[bc].ls_eps : el.e[c];
        const QuadOut q = wbq_rollout_knot<QDL>(*Pc, md, bc, kc, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, c == el.writer, in);
        if ((t & 3) == 0) {
            const size_t slot = ((size_t)c * batch + bc) * nslots + s;
            sa.cost[slot] = q.cost; sa.dsq[slot] = q.dsq; sa.ming[slot] = q.ming; sa.maxh[slot] = 0.0;
            if (q.bad) fail[(size_t)c * batch + bc] = 1;
        }
    }
}

void launch_k_rollout_quad(unsigned grid, hipStream_t stream, const PhaseDev* ph, const int* slot_phase, const int* slot_k, const int* qslots, int nq, int nslots, int batch,
                           ModelDev md, EpsList el, OptDev opt, const double* x0, SlotArrays sa, const ProbState* st, int mask, int* fail, unsigned long long* units,
                           const int* plist, int nlist) {
    hipLaunchKernelGGL(k_rollout_quad, dim3(grid), dim3(64), 0, stream, ph, slot_phase, slot_k, qslots, nq, nslots, batch, md, el, opt, x0, sa, st, mask, fail, units, plist, nlist);
}

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

void launch_k_rollout_quad_term(unsigned grid, hipStream_t stream, const PhaseDev* ph, int nph, const int* slot_phase, const int* tslots, int nslots, int batch,
                                ModelDev md, EpsList el, OptDev opt, SlotArrays sa, const ProbState* st, int mask, const int* plist, int nlist) {
    hipLaunchKernelGGL(k_rollout_quad_term, dim3(grid), dim3(64), 0, stream, ph, nph, slot_phase, tslots, nslots, batch, md, el, opt, sa, st, mask, plist, nlist);
}

#ifdef QUAD_PROF
extern "C"
int hsddp_debug_quad_prof(unsigned long long* out24, int reset) {
    hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_quad_prof), 24 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[24] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_quad_prof), z, sizeof(z)); }
    return 0;
}
#endif
