// TEST-ONLY host build of the whole-body programs WITH per-problem cost-weight scales (include/hsddp_weights.h) under the lane emulator: the one-wave
// rollout knot, terminal knot, LQ knot and terminal LQ (wb_knot.hpp) and the lane-quad knot and terminal knot (wb_quad.hpp, wb_quad_term.hpp: the
// four lanes of a quad as a four-wide value), each with the PW switch on and the problem's row as the extra operand - and of k_pack_weights' loop
// and the argument rules (weights.hpp).  It takes the whole emulator as term_emu.cpp does (emu.cpp: the handle, the ABI of include/hsddp.h, the
// per-step entry points) and adds the entry points below; the steps that read no weight (sweep, linear rollout, nominal update) are emu.cpp's.
// tests/pw_common.py builds and binds it.
#include "term_emu.cpp"
#define WEIGHTS_HOST_ONLY 1
#include "weights.hpp"

// the launch rule of roll_pick / lq_pick (roll_pick.hpp): with scales every whole-body knot runs the PW program with row b of the table;
// the terminal programs have the touchdown heights compiled in and read the phase's ground_height from a table when the phase has none of its own
static void pw_chain(hsddp_handle* h, const std::vector<PhaseDev>& ph, WbCore& L, int first, int b, double eps, const OptDev& o, SlotOut so, const double* ws) {
    for (int pj = first; pj < h->nph && !ph[pj].shooting; pj++) {
        const PhaseDev& Q = ph[pj]; const PhaseDev* Qn = pj + 1 < h->nph ? &ph[pj + 1] : nullptr; const size_t s0 = (size_t)b * h->nslots + Q.slot0;
        if (Q.model == HSDDP_MODEL_WB) {
            const double gh[4] = {Q.ground_height, Q.ground_height, Q.ground_height, Q.ground_height};
            for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64, true>(L, Q, h->md, b, kq, eps, o.ReB_active, nullptr, so, s0 + kq, h->fail.data(), true, true, ws);
            wb_rollout_terminal<64, true, true>(L, Q, Qn, h->md, b, eps, o.AL_active, so, s0 + Q.h, true, true, gh, ws);
        } else if (Q.model == HSDDP_MODEL_SRB) {
            SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
            for (int kq = 0; kq < Q.h; kq++) srb_rollout_knot<64>(Ls, Q, b, kq, eps, o.ReB_active, nullptr, so, s0 + kq, h->fail.data(), true);
            srb_rollout_terminal<64>(Ls, Q, Qn, b, eps, so, s0 + Q.h, true);
        } else {
            HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
            for (int kq = 0; kq < Q.h; kq++) hkd_rollout_knot<64>(Lh, Q, b, kq, eps, o.ReB_active, nullptr, so, s0 + kq, h->fail.data(), true);
            hkd_rollout_terminal<64>(Lh, Q, Qn, h->md, b, eps, o.AL_active, so, s0 + Q.h, true);
        }
    }
}

extern "C" {
// hsddp_hybrid_rollout with scales [batch][84] (null: emu.cpp's entry point, the programs without the switch).  program 0: the one-wave programs
// everywhere (HSDDP_QUAD=0 HSDDP_QUAD_TERMINAL=0); 1: the lane-quad knot for the running knots of whole-body phases with shooting nodes and the
// lane-quad terminal knot for the terminal slots split_slots gives it, the one-wave programs for the rest (the default launch).
int pw_emu_hybrid_rollout(hsddp_handle_t* h, double eps, const hsddp_option_t* opt, const double* scales, int program) {
    if (scales == nullptr) return hsddp_hybrid_rollout(h, eps, opt);
    OptDev o = to_dev(*opt); SlotOut so{h->cost.data(), h->dsq.data(), h->ming.data(), h->maxh.data()};
    static WbCore L;
    std::vector<PhaseDev> ph = h->ph;
    if (!o.MS) for (auto& q : ph) q.shooting = 0;
    const bool quad = program == 1 && o.MS;
    for (int b = 0; b < h->batch; b++) {
        const double* ws = scales + (size_t)b * WS_ROW;
        h->fail[b] = 0;
        if (!ph[0].shooting) {
            const int n0 = ph[0].n;
            if (ph[0].model == HSDDP_MODEL_WB) for (int i = 0; i < 36; i++) L.xnext[i] = h->x0[(size_t)b * 36 + i];
            else for (int i = 0; i < n0; i++) ph[0].Xsim[(size_t)b * (ph[0].h + 1) * n0 + i] = h->x0[(size_t)b * n0 + i];
            pw_chain(h, ph, L, 0, b, eps, o, so, ws);
        } else for (int s = 0; s < h->nslots; s++) {
            int pi = h->sp[s], k = h->sk[s]; const PhaseDev& P = ph[pi]; size_t slot = (size_t)b * h->nslots + s;
            const PhaseDev* Pn = pi + 1 < h->nph ? &ph[pi + 1] : nullptr;
            if (!P.shooting) continue;
            if (P.model == HSDDP_MODEL_HKD) {
                HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
                if (k < P.h) hkd_rollout_knot<64>(Lh, P, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data());
                else { hkd_rollout_terminal<64>(Lh, P, Pn, h->md, b, eps, o.AL_active, so, slot); pw_chain(h, ph, L, pi + 1, b, eps, o, so, ws); }
            } else if (P.model == HSDDP_MODEL_SRB) {
                SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
                if (k < P.h) srb_rollout_knot<64>(Ls, P, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data());
                else { srb_rollout_terminal<64>(Ls, P, Pn, b, eps, so, slot); pw_chain(h, ph, L, pi + 1, b, eps, o, so, ws); }
            } else {
                const double gh[4] = {P.ground_height, P.ground_height, P.ground_height, P.ground_height};
                if (k < P.h && quad) {
                    const QuadOut q = wbq_rollout_knot<QH, true>(P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, true, ws);
                    so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = q.ming; so.maxh[slot] = 0.0; if (q.bad) h->fail[b] = 1;
                } else if (k < P.h) wb_rollout_knot<64, true>(L, P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data(), false, true, ws);
                else if (quad && term_owned(h, pi)) {
                    const QuadTermOut q = wbq_rollout_terminal<QH, true, true>(P, Pn, h->md, b, eps, o.AL_active, true, gh, ws);
                    so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = 0.0; so.maxh[slot] = q.maxh;
                } else { wb_rollout_terminal<64, true, true>(L, P, Pn, h->md, b, eps, o.AL_active, so, slot, false, true, gh, ws); pw_chain(h, ph, L, pi + 1, b, eps, o, so, ws); }
            }
        }
        double c = 0, d = 0; for (int s = 0; s < h->nslots; s++) { c += h->cost[(size_t)b * h->nslots + s]; d += h->dsq[(size_t)b * h->nslots + s]; }
        h->acost[b] = c; h->feas[b] = sqrt(d);
    }
    h->cache_valid = true;
    return 0;
}
// hsddp_LQ_approximation with scales [batch][84] (null: emu.cpp's entry point)
int pw_emu_LQ_approximation(hsddp_handle_t* h, const hsddp_option_t* opt, const double* scales) {
    if (scales == nullptr) return hsddp_LQ_approximation(h, opt);
    OptDev o = to_dev(*opt); static WbLqLds L; static SrbLds Ls; static HkdLds Lh;
    for (int b = 0; b < h->batch; b++) for (int s = 0; s < h->nslots; s++) {
        int pi = h->sp[s], k = h->sk[s]; const PhaseDev& P = h->ph[pi]; const PhaseDev* Pn = pi + 1 < h->nph ? &h->ph[pi + 1] : nullptr;
        const double* ws = scales + (size_t)b * WS_ROW;
        if (P.model == HSDDP_MODEL_HKD) { if (k < P.h) hkd_lq_knot<EMU_LQ_NT>(Lh, P, b, k, o.ReB_active); else hkd_lq_terminal<EMU_LQ_NT>(Lh, P, Pn, h->md, b, o.AL_active); }
        else if (P.model == HSDDP_MODEL_SRB) { if (k < P.h) srb_lq_knot<EMU_LQ_NT>(Ls, P, b, k, o.ReB_active); else srb_lq_terminal<EMU_LQ_NT>(Ls, P, Pn, b); }
        else if (k < P.h) wb_lq_knot<EMU_LQ_NT, true>(L, P, h->md, b, k, o.ReB_active, h->cache_valid, ws);
        else wb_lq_terminal<EMU_LQ_NT, true>(L, P, Pn, h->md, b, o.AL_active, ws);
    }
    return 0;
}
// k_pack_weights' loop on the host (weights.hpp): the table [batch][84], the caller's rows [nb][84] for [b0, b0+nb), `first` as hsddp_weights_set sees it
int pw_emu_pack(double* table, int batch, const double* src, int b0, int nb, int first) {
    const hs::WsPack W{table, src, b0, nb, first ? 0 : b0, first ? batch : nb};
    hs::ws_pack_host(W);
    return 0;
}
// the argument rules (weights.hpp) as the library applies them
int pw_emu_check_set(int batch, int f32, int b0, int nb, const double* scales, int src_device) { return hs::ws_check_set(hs::WsHandleInfo{batch, f32}, b0, nb, scales, src_device); }
int pw_emu_check_range(int batch, int f32, int b0, int nb) { return hs::ws_check_range(hs::WsHandleInfo{batch, f32}, b0, nb); }
}
