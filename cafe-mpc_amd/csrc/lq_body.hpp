// The LQ-approximation program of libhsddp_hip.so: what k_lq / k_lq_hkd (hsddp_hip.hip) and k_lq_pw (hsddp_pw.hip) are instantiated from.  A header
// of its own because hsddp_pw.hip is compiled as a translation unit of its own by the Makefile; hsddp_hip.hip includes it where the text used to
// stand.  PW (default off): per-problem cost-weight scales (hsddp_weights.h) - wtab is the handle's table [batch][84] and the whole-body knots of
// problem b read row b of it; single-rigid-body and kinodynamic knots never do.  LIM (default off, with PW on): per-problem constraint limits
// (hsddp_limits.h) - ltab is the handle's resolved table [phase][batch][12]; the running knots read mu of row (phase, b).
#pragma once
#include "hsddp.h"
#include "hs_types.hpp"
#include "wb_knot.hpp"
#include "srb_knot.hpp"
#include "hkd_knot.hpp"
#include "rollout_args.hpp"

using namespace hs;

// LQ workgroup: 128 threads = two waves per knot (tangent rounds side by side, then column solves || cost partials), capped at 256
// registers so that the four knots a CU holds in LDS make two waves per SIMD.  LQ_NT=64 is the one-wave variant.
#ifndef LQ_NT
#define LQ_NT 128
#endif
#ifndef LQ_WPE
#define LQ_WPE 2
#endif
#define LQ_ATTR __attribute__((amdgpu_waves_per_eu(LQ_WPE, LQ_WPE)))

#define LQ_ARGS const PhaseDev* ph_, int nph, const int* slot_phase, const int* slot_k, int nslots, ModelDev md, OptDev opt, const ProbState* st, int mask, int use_cache, unsigned long long* units
template <bool WBM, int NT, bool PW = false, bool LIM = false, class LDS> __device__ __forceinline__ void lq_body(LDS& L, LQ_ARGS, const double* wtab = nullptr, const double* ltab = nullptr, int batch = 0) {
    static_assert(!LIM || PW, "the program with limits has the scales compiled in");
    PhaseC* ph = (PhaseC*)ph_;   // descriptors: constant memory, scalar loads
    const int b = blockIdx.x / nslots, s = blockIdx.x % nslots;
    if (masked_out(st[b], mask)) return;
    if (s == 0 && threadIdx.x == 0) atomicAdd(units, (unsigned long long)nslots - nph);
    const int pi = slot_phase[s], k = slot_k[s];
    PhaseC& P = ph[pi];
    if (P.model == HSDDP_MODEL_HKD) {
        HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
        if (k < P.h) hkd_lq_knot<NT>(Lh, P, b, k, opt.ReB_active); else hkd_lq_terminal<NT>(Lh, P, pi + 1 < nph ? &ph[pi + 1] : nullptr, md, b, opt.AL_active);
        return;
    }
    if (P.model == HSDDP_MODEL_SRB) {
        SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
        if (k < P.h) srb_lq_knot<NT>(Ls, P, b, k, opt.ReB_active); else srb_lq_terminal<NT>(Ls, P, pi + 1 < nph ? &ph[pi + 1] : nullptr, b);
        return;
    }
    if constexpr (LIM) {      // (b and pi are uniform over the workgroup: so are both row pointers)
        WsRow ws = (WsRow)wtab + (size_t)b * WS_ROW;
        if (k < P.h) wb_lq_knot<NT, true, true>(L, P, md, b, k, opt.ReB_active, use_cache != 0, ws, (LimRow)ltab + ((size_t)pi * batch + b) * LIM_ROW);
        else wb_lq_terminal<NT, true>(L, P, pi + 1 < nph ? &ph[pi + 1] : nullptr, md, b, opt.AL_active, ws);
    } else if constexpr (PW) {      // (b comes from blockIdx: the row pointer is uniform over the workgroup)
        WsRow ws = (WsRow)wtab + (size_t)b * WS_ROW;
        if (k < P.h) wb_lq_knot<NT, true>(L, P, md, b, k, opt.ReB_active, use_cache != 0, ws);
        else wb_lq_terminal<NT, true>(L, P, pi + 1 < nph ? &ph[pi + 1] : nullptr, md, b, opt.AL_active, ws);
    } else if constexpr (WBM) {
        if (k < P.h) wb_lq_knot<NT>(L, P, md, b, k, opt.ReB_active, use_cache != 0);
        else wb_lq_terminal<NT>(L, P, pi + 1 < nph ? &ph[pi + 1] : nullptr, md, b, opt.AL_active);
    }
}
#define LQ_PASS ph_, nph, slot_phase, slot_k, nslots, md, opt, st, mask, use_cache, units
