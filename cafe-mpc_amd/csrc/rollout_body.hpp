// The one-wave rollout program of libhsddp_hip.so: what k_rollout / k_rollout_hkd (hsddp_hip.hip) and k_rollout_tdh (hsddp_tdh.hip) are instantiated
// from.  A header of its own because hsddp_tdh.hip is compiled as a translation unit of its own by the Makefile; hsddp_hip.hip includes it where the
// text used to stand.  TDH (default off): per-problem touchdown heights (hsddp_touchdown.h) - tdh is the window's table [phase][batch][4] and the
// terminal knots of whole-body phases read their row of it instead of the descriptor's ground_height.  PW (default off): per-problem cost-weight
// scales (hsddp_weights.h) - wtab is the handle's table [batch][84] and the whole-body knots of problem b read row b of it; the instantiation with PW
// has TDH compiled in as well (hsddp_pw.hip).  LIM (default off): per-problem constraint limits (hsddp_limits.h) - ltab is the handle's resolved table
// [phase][batch][12] and the running knots of whole-body phase i of problem b read row (i, b) of it; the instantiation with LIM has PW and TDH
// compiled in (hsddp_lim.hip).
#pragma once
#include "hsddp.h"
#include "hs_types.hpp"
#include "wb_knot.hpp"
#include "srb_knot.hpp"
#include "hkd_knot.hpp"
#include "rollout_args.hpp"

using namespace hs;

#ifndef ROLL_ATTR
#ifdef ROLL_WPE
#define ROLL_ATTR __attribute__((amdgpu_waves_per_eu(ROLL_WPE, ROLL_WPE)))
#else
#define ROLL_ATTR
#endif
#endif

// Single shooting from phase `first` on, by ONE wave: every knot takes the state its predecessor simulated (SinglePhase.cpp:187,211-220).
// Used for the young phases the receding-horizon update creates (SS_set empty, MHPCProblem.cpp:340-351; first > 0, stops at the next
// phase with shooting nodes) and for the whole horizon when option.MS is false (MultiPhaseDDP.cpp:65-68; first = 0, descriptors with
// every shooting flag cleared).  On entry the state to start from is in L.xnext (whole-body phase) / in Xsim[0] of the phase (SRB, HKD).
template <bool WBM, bool TDH = false, bool PW = false, bool LIM = false, class LDS> __device__ __forceinline__ void rollout_chain(LDS& L, PhaseC* ph, int nph, int first, const ModelDev& md, int b, int nslots, double eps, const OptDev& opt, SlotOut so,
                                              size_t slot_base, int* fail, bool wr, const double* tdh = nullptr, int batch = 0, WsRow ws = nullptr, const double* ltab = nullptr) {
    for (int pj = first; pj < nph && !ph[pj].shooting; pj++) {
        PhaseC& Q = ph[pj]; PhaseC* Qn = pj + 1 < nph ? &ph[pj + 1] : nullptr; const size_t s0 = slot_base + Q.slot0;
        if (WBM && Q.model == HSDDP_MODEL_WB) {
            if constexpr (WBM) {
            if constexpr (LIM) {
                LimRow lim = (LimRow)ltab + ((size_t)pj * batch + b) * LIM_ROW;
                for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64, true, true>(L, Q, md, b, kq, eps, opt.ReB_active, nullptr, so, s0 + kq, fail, true, wr, ws, lim);
                wb_rollout_terminal<64, true, true>(L, Q, Qn, md, b, eps, opt.AL_active, so, s0 + Q.h, true, wr, tdh + ((size_t)pj * batch + b) * 4, ws);
            } else if constexpr (PW) {
                for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64, true>(L, Q, md, b, kq, eps, opt.ReB_active, nullptr, so, s0 + kq, fail, true, wr, ws);
                wb_rollout_terminal<64, true, true>(L, Q, Qn, md, b, eps, opt.AL_active, so, s0 + Q.h, true, wr, tdh + ((size_t)pj * batch + b) * 4, ws);
            } else {
            for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64>(L, Q, md, b, kq, eps, opt.ReB_active, nullptr, so, s0 + kq, fail, true, wr);
            if constexpr (TDH) wb_rollout_terminal<64, true>(L, Q, Qn, md, b, eps, opt.AL_active, so, s0 + Q.h, true, wr, tdh + ((size_t)pj * batch + b) * 4);
            else wb_rollout_terminal<64>(L, Q, Qn, md, b, eps, opt.AL_active, so, s0 + Q.h, true, wr);
            }
            }
        } else if (Q.model == HSDDP_MODEL_SRB) {      // (reads the simulated state back from Xsim: not available to probes, see hsddp_solve)
            SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
            for (int kq = 0; kq < Q.h; kq++) srb_rollout_knot<64>(Ls, Q, b, kq, eps, opt.ReB_active, nullptr, so, s0 + kq, fail, true, wr);
            srb_rollout_terminal<64>(Ls, Q, Qn, b, eps, so, s0 + Q.h, true, wr);
        } else {
            HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
            for (int kq = 0; kq < Q.h; kq++) hkd_rollout_knot<64>(Lh, Q, b, kq, eps, opt.ReB_active, nullptr, so, s0 + kq, fail, true, wr);
            hkd_rollout_terminal<64>(Lh, Q, Qn, md, b, eps, opt.AL_active, so, s0 + Q.h, true, wr);
        }
    }
}

// Probe launches of the ONE-WAVE kernels (k_rollout, k_rollout_hkd; the quad kernel loops over the candidates inside a unit's wave instead):
// grid = candidates x units.  Workgroups go round-robin over the 8 XCDs (one L2 each); the candidates of a unit read the same
// trajectories and differ in eps only.  Unit u lives on XCD u % 8 and its candidates occupy consecutive dispatch slots of that XCD, so one of them
// brings the lines into that L2 and the others find them there (candidate-major order streamed the whole ensemble from HBM once per candidate:
// probe launch of the quad kernel 11.4 -> 9.8 ms).  QUAD_CAND_MAJOR 1 = the old order.
#ifndef QUAD_CAND_MAJOR
#define QUAD_CAND_MAJOR 0
#endif
__device__ __forceinline__ void cand_unit(int per, int g, int& c, int& r) {
#if QUAD_CAND_MAJOR
    c = g / per; r = g - c * per;
#else
    const int ncand = gridDim.x / per;
    const int full = (per >> 3) << 3;
    if (g < full * ncand) { const int G = g / (8 * ncand), rem = g - G * 8 * ncand; c = rem >> 3; r = G * 8 + (rem & 7); }
    else { const int nt = per - full, g2 = g - full * ncand; c = g2 / nt; r = full + (g2 - c * nt); }
#endif
}

// LDS of the kernels instantiated WITHOUT the whole-body model (kinodynamic / single-rigid-body handles): 8 KB instead of 16 / 40 KB, so that
// their small knots are not held to the whole-body kernels' two waves per SIMD
union RedLds { HkdLds h; SrbLds s; };
// slot_list / nlist: the slots this launch covers (null: all nslots) - when the lane-quad kernel takes the whole-body running knots of a launch,
// the one-wave programs only see the rest (the terminal knots it leaves with their reset maps, single-rigid-body knots); unit_knots: running knots
// among them; plist / nprob: the problems this launch is for (null: all nprob = batch of them, `mask` picks)
#define ROLL_ARGS const PhaseDev* ph_, int nph, const int* slot_phase, const int* slot_k, int nslots, int batch, ModelDev md, EpsList el, OptDev opt, const double* x0, SlotArrays sa, \
                  const ProbState* st, int mask, int* fail, unsigned long long* units, const int* slot_list, int nlist, int unit_knots, const int* plist, int nprob
template <bool WBM, bool TDH = false, bool PW = false, bool LIM = false, class LDS> __device__ __forceinline__ void rollout_body(LDS& L, ROLL_ARGS, const double* tdh = nullptr, const double* wtab = nullptr, const double* ltab = nullptr) {
    static_assert(!PW || (WBM && TDH), "the scaled program is the whole-body one with the touchdown heights compiled in");
    static_assert(!LIM || PW, "the program with limits has the scales and the touchdown heights compiled in");
    PhaseC* ph = (PhaseC*)ph_;   // descriptors: constant memory, scalar loads
    const int per = nprob * nlist;
    int c, r; cand_unit(per, blockIdx.x, c, r);
    const int ip = r / nlist, si = r - ip * nlist;
    const int b = plist != nullptr ? plist[ip] : ip;
    if (masked_out(st[b], mask)) return;
    if (si == 0 && threadIdx.x == 0) atomicAdd(units, (unsigned long long)unit_knots);     // knots this launch rolls out (measurement only)
    const int s = slot_list != nullptr ? slot_list[si] : si;
    const int pi = slot_phase[s], k = slot_k[s];
    PhaseC& P = ph[pi];
    const size_t cbase = (size_t)c * batch * nslots;            // slice of candidate c in the slot arrays
    SlotOut so{sa.cost, sa.dsq, sa.ming, sa.maxh};
    const size_t slot_base = cbase + (size_t)b * nslots, slot = slot_base + s;
    const double eps = el.from_state ? st[b].ls_eps : el.e[c];
    const bool wr = (c == el.writer);
    fail += (size_t)c * batch;
    int chain_first = -1;
    if (!ph[0].shooting) {       // single shooting over the whole horizon (option.MS = false): the wave of slot 0 walks every phase
        if (s != 0) return;
        const int n0 = ph[0].n;
        if (WBM && ph[0].model == HSDDP_MODEL_WB) { if constexpr (WBM) { HS_PHASE(64, if (tid < 36) L.xnext[tid] = x0[(size_t)b * 36 + tid];) } }
        else { HS_PHASE(64, if (tid < n0) ph[0].Xsim[(size_t)b * (ph[0].h + 1) * n0 + tid] = x0[(size_t)b * n0 + tid];) }
        chain_first = 0;
    } else {
        if (!P.shooting) return;     // a phase without shooting nodes is rolled sequentially by the wave of its predecessor's terminal knot
        PhaseC* Pn = pi + 1 < nph ? &ph[pi + 1] : nullptr;
        if (k == P.h) chain_first = pi + 1;
        if (P.model == HSDDP_MODEL_HKD) {
            HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
            if (k < P.h) hkd_rollout_knot<64>(Lh, P, b, k, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, so, slot, fail, false, wr);
            else hkd_rollout_terminal<64>(Lh, P, Pn, md, b, eps, opt.AL_active, so, slot, false, wr);
        } else if (P.model == HSDDP_MODEL_SRB) {   // reduced-model tail of the MHPC horizon: a few hundred flops per knot, reuses the whole-body LDS block
            SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
            if (k < P.h) srb_rollout_knot<64>(Ls, P, b, k, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, so, slot, fail, false, wr);
            else srb_rollout_terminal<64>(Ls, P, Pn, b, eps, so, slot, false, wr);
        } else if constexpr (LIM) {      // (b and pi are uniform over the wave: so are both row pointers)
            WsRow ws = (WsRow)wtab + (size_t)b * WS_ROW;
            if (k < P.h) wb_rollout_knot<64, true, true>(L, P, md, b, k, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, so, slot, fail, false, wr, ws, (LimRow)ltab + ((size_t)pi * batch + b) * LIM_ROW);
            else wb_rollout_terminal<64, true, true>(L, P, Pn, md, b, eps, opt.AL_active, so, slot, false, wr, tdh + ((size_t)pi * batch + b) * 4, ws);
        } else if constexpr (PW) {      // (b comes from blockIdx: the row pointer is uniform over the wave)
            WsRow ws = (WsRow)wtab + (size_t)b * WS_ROW;
            if (k < P.h) wb_rollout_knot<64, true>(L, P, md, b, k, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, so, slot, fail, false, wr, ws);
            else wb_rollout_terminal<64, true, true>(L, P, Pn, md, b, eps, opt.AL_active, so, slot, false, wr, tdh + ((size_t)pi * batch + b) * 4, ws);
        } else if constexpr (WBM) {
            if (k < P.h) wb_rollout_knot<64>(L, P, md, b, k, eps, opt.ReB_active, pi == 0 ? x0 : nullptr, so, slot, fail, false, wr);
            else if constexpr (TDH) wb_rollout_terminal<64, true>(L, P, Pn, md, b, eps, opt.AL_active, so, slot, false, wr, tdh + ((size_t)pi * batch + b) * 4);
            else wb_rollout_terminal<64>(L, P, Pn, md, b, eps, opt.AL_active, so, slot, false, wr);
        }
    }
    // single-shooting phases from here on (young phases behind a terminal knot, or the whole horizon): ONE call site, one copy of the code
    if (chain_first >= 0 && chain_first < nph && !ph[chain_first].shooting) {
        if constexpr (LIM) rollout_chain<WBM, true, true, true>(L, ph, nph, chain_first, md, b, nslots, eps, opt, so, slot_base, fail, wr, tdh, batch, (WsRow)wtab + (size_t)b * WS_ROW, ltab);
        else if constexpr (PW) rollout_chain<WBM, true, true>(L, ph, nph, chain_first, md, b, nslots, eps, opt, so, slot_base, fail, wr, tdh, batch, (WsRow)wtab + (size_t)b * WS_ROW);
        else if constexpr (TDH) rollout_chain<WBM, true>(L, ph, nph, chain_first, md, b, nslots, eps, opt, so, slot_base, fail, wr, tdh, batch);
        else rollout_chain<WBM>(L, ph, nph, chain_first, md, b, nslots, eps, opt, so, slot_base, fail, wr);
    }
}
#define ROLL_PASS ph_, nph, slot_phase, slot_k, nslots, batch, md, el, opt, x0, sa, st, mask, fail, units, slot_list, nlist, unit_knots, plist, nprob
