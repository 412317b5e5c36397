// What k_rollout_quad_term (hsddp_quad.hip) and k_rollout_quad_term_tdh (hsddp_tdh.hip) share: the row layout of the lane-quad kernels' LDS stage and
// the terminal kernel's body.  TDH: per-problem touchdown heights (hsddp_touchdown.h), tdh = the window's table [phase][batch][4]; the lane reads
// the height of its own leg.  `stage` is the kernel's __shared__ block of 16 x QS_ROW doubles.
#pragma once
#include <hip/hip_runtime.h>
#include "hs_types.hpp"
#include "wb_quad.hpp"
#include "wb_quad_term.hpp"
#include "rollout_args.hpp"

#ifndef QUAD_WPE
#define QUAD_WPE 1      // waves per SIMD the quad kernel is compiled for (1: up to 512 registers, nothing in scratch; 2: 256 registers)
#endif
constexpr int QS_DX = 72, QS_U = 144, QS_DU = 156, QS_KDX = 168, QS_RR = 180, QS_ROW = 268;
// PW: per-problem cost-weight scales (hsddp_weights.h), wtab = the handle's table [batch][84]; the lane reads the row of its quad's problem (with TDH on).
template <bool TDH, bool PW = false>
__device__ __forceinline__ void quad_term_body(double* stage, const hs::PhaseDev* ph_, int nph, const int* slot_phase, const int* tslots, int nslots, int batch, hs::ModelDev md, EpsList el,
                                               hs::OptDev opt, SlotArrays sa, const hs::ProbState* st, int mask, const int* plist, int nlist, const double* tdh, const double* wtab = nullptr) {
    static_assert(!PW || TDH, "the scaled terminal program has the touchdown heights compiled in");
    using namespace hs;
    PhaseC* ph = (PhaseC*)ph_;
    const int nprob = plist != nullptr ? nlist : batch;
    const int nbg = (nprob + 15) >> 4;
    const int qi = blockIdx.x / nbg, bg = blockIdx.x - qi * nbg;
    const int s = tslots[qi], pi = slot_phase[s];
    const bool hasn = pi + 1 < nph;
    PhaseC& P = ph[pi];
    PhaseC& N = ph[hasn ? pi + 1 : pi];
    const int t = threadIdx.x;
    const int ix = bg * 16 + (t >> 2);
    const int b = ix < nprob ? (plist != nullptr ? plist[ix] : ix) : batch;
    const bool active = b < batch && !masked_out(st[b < batch ? b : 0], mask);
    if (__ballot(active) == 0) return;      // none of the wave's problems takes part in this launch: nothing to stage
    {   // stage the rows of the wave's sixteen problems: per problem three whole-wave loads (Xbar, dX: lanes 0..35 knot h, lanes 36..63 entries 0..27
        // of the successor's knot 0; reference row: entries 0..63) and one that gathers the tails; all of them issued before the first is written
        // to LDS.  A group that is only partly filled stages its last problem again in the empty places: nothing is read beyond the list or the batch.
        const int h = P.h;
        const bool own = t < 36;
        const HS_GLOBAL double *pX = own ? P.Xbar : N.Xbar, *pdX = own ? P.dX : N.dX, *pR = P.rref;
        const unsigned nmul = (unsigned)(N.h + 1) * 36u, rmul = (unsigned)P.ref_pb * 80u;
        const unsigned xmul = own ? (unsigned)(h + 1) * 36u : nmul;
        const size_t xadd = own ? (size_t)h * 36 + t : (size_t)(t - 36);
        const int seg = t < 8 ? 0 : t < 16 ? 1 : t < 28 ? 2 : 3;      // tail of the successor's Xbar[0], dX[0] (entries 28..35), reference row (64..75); the other lanes load a dummy
        const HS_GLOBAL double* tsrc = seg == 0 ? N.Xbar : seg == 1 ? N.dX : pR;
        const unsigned tmul = seg < 2 ? nmul : rmul;
        const size_t tadd = seg == 0 ? (size_t)(28 + t) : seg == 1 ? (size_t)(28 + (t - 8)) : seg == 2 ? (size_t)h * 80 + 64 + (t - 16) : (size_t)h * 80;
        const int tdst = seg == 0 ? 64 + t : seg == 1 ? QS_DX + 64 + (t - 8) : seg == 2 ? QS_RR + 64 + (t - 16) : QS_U + (t - 28);      // (QS_U .. QS_RR: unused by the terminal knot)
        const int ixl = min(bg * 16 + (t & 15), nprob - 1);
        const int bl = plist != nullptr ? plist[ixl] : ixl;      // lane p (mod 16) holds problem p of the group
        double v[16][4];
        _Pragma("unroll")
        for (int p = 0; p < 16; p++) {
            const int bp = __builtin_amdgcn_readlane(bl, p);
            const size_t kr = ref_row(P, bp, h) * 80;
            v[p][0] = pX[(size_t)bp * xmul + xadd]; v[p][1] = pdX[(size_t)bp * xmul + xadd]; v[p][2] = pR[kr + t]; v[p][3] = tsrc[(size_t)bp * tmul + tadd];
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
    for (int c = 0; c < el.n; c++) {      // as in k_rollout_quad: nothing a trip derives from its descriptors, problem or row may be carried across the loop
        PhaseC* Pc = &P; HS_PIN_S(Pc);
        PhaseC* Nc = &N; HS_PIN_S(Nc);
        int bc = b;
        int ro = (t >> 2) * QS_ROW; HS_PIN(bc); HS_PIN(ro);
        const HS_LDS double* row = (const HS_LDS double*)stage + ro;
        const QuadIn<const HS_LDS double*> in = {row, row + QS_DX, row + QS_U, row + QS_DU, row + QS_KDX, row + QS_RR};
        const double eps = el.from_state ? st[bc].ls_eps : el.e[c];
        QuadTermOut q;
        if constexpr (PW) q = wbq_rollout_terminal<QDL, true, true>(*Pc, hasn ? Nc : nullptr, md, bc, eps, opt.AL_active, c == el.writer, in, tdh + ((size_t)pi * batch + bc) * 4,
                                                                    (hs::WsRow)wtab + (size_t)bc * hs::WS_ROW);
        else if constexpr (TDH) q = wbq_rollout_terminal<QDL, true>(*Pc, hasn ? Nc : nullptr, md, bc, eps, opt.AL_active, c == el.writer, in, tdh + ((size_t)pi * batch + bc) * 4);
        else q = wbq_rollout_terminal<QDL>(*Pc, hasn ? Nc : nullptr, md, bc, eps, opt.AL_active, c == el.writer, in);
        if ((t & 3) == 0) {
            const size_t slot = ((size_t)c * batch + bc) * nslots + s;
            sa.cost[slot] = q.cost; sa.dsq[slot] = q.dsq; sa.ming[slot] = 0.0; sa.maxh[slot] = q.maxh;
        }
    }
}
