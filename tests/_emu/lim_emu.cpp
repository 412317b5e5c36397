// TEST-ONLY host build of the whole-body programs WITH per-problem constraint limits (include/hsddp_limits.h) under the lane emulator: the one-wave
// rollout knot and LQ knot (wb_knot.hpp) and the lane-quad knot (wb_quad.hpp: the four lanes of a quad as a four-wide value), each with the LIM
// switch on and the problem's resolved row as the extra operand - and of k_pack_limits' and k_lim_mu's loops and the argument rules
// (limits.hpp).  It takes pw_emu.cpp (the emulator, the terminal programs, the programs with cost-weight scales) and adds the entry points below; the
// steps that read no limit (sweep, linear rollout, nominal update) are emu.cpp's.  tests/lim_common.py builds and binds it.
#include "pw_emu.cpp"
#define LIMITS_HOST_ONLY 1
#include "limits.hpp"

static_assert(hs::LMP_ROW == LIM_ROW && hs::LMP_TORQUE == LIM_TORQUE && hs::LMP_JLB == LIM_JLB && hs::LMP_JUB == LIM_JUB && hs::LMP_HMIN == LIM_HMIN && hs::LMP_MU == LIM_MU &&
              hs::LMP_JSLB == LIM_JSLB && hs::LMP_JSUB == LIM_JSUB, "one row layout");

// the limits of a phase descriptor as a row (lim_desc_row, limits_host.hpp)
static void lim_row_of(const PhaseDev& P, double* r) {
    r[LIM_TORQUE] = P.torque_limit;
    for (int j = 0; j < 3; j++) { r[LIM_JLB + j] = P.joint_lb[j]; r[LIM_JUB + j] = P.joint_ub[j]; }
    r[LIM_HMIN] = P.h_min; r[LIM_MU] = P.mu; r[LIM_JSLB] = P.jspeed_lb; r[LIM_JSUB] = P.jspeed_ub; r[11] = 0.0;
}
// the resolved table [nph][batch][12] of the handle's window from user rows [batch][12], through k_pack_limits' loop
static std::vector<double> lim_resolve(const hsddp_handle* h, const double* user) {
    std::vector<double> desc((size_t)h->nph * LIM_ROW), res((size_t)h->nph * h->batch * LIM_ROW, -7.0), u(user, user + (size_t)h->batch * LIM_ROW);
    for (int i = 0; i < h->nph; i++) lim_row_of(h->ph[i], desc.data() + (size_t)i * LIM_ROW);
    hs::lim_pack_host(hs::LimPack{u.data(), res.data(), nullptr, desc.data(), h->batch, h->nph, 0, 0, 0, h->batch, hs::LIM_PACK_RESOLVE});
    return res;
}

// the launch rule of roll_pick / lq_pick (roll_pick.hpp): with limits every whole-body running knot runs the LIM program with row (phase, b)
// of the resolved table and a scale row (ones while no scales are set); the one-wave terminal program is the scaled one with the heights compiled in
static void lim_chain(hsddp_handle* h, const std::vector<PhaseDev>& ph, WbCore& L, int first, int b, double eps, const OptDev& o, SlotOut so, const double* ws, const double* res) {
    for (int pj = first; pj < h->nph && !ph[pj].shooting; pj++) {
        const PhaseDev& Q = ph[pj]; const PhaseDev* Qn = pj + 1 < h->nph ? &ph[pj + 1] : nullptr; const size_t s0 = (size_t)b * h->nslots + Q.slot0;
        if (Q.model == HSDDP_MODEL_WB) {
            const double gh[4] = {Q.ground_height, Q.ground_height, Q.ground_height, Q.ground_height};
            if (res == nullptr) {      // no table: the programs without switches
                for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64>(L, Q, h->md, b, kq, eps, o.ReB_active, nullptr, so, s0 + kq, h->fail.data(), true, true);
                wb_rollout_terminal<64>(L, Q, Qn, h->md, b, eps, o.AL_active, so, s0 + Q.h, true, true);
                continue;
            }
            const double* lim = res + ((size_t)pj * h->batch + b) * LIM_ROW;
            for (int kq = 0; kq < Q.h; kq++) wb_rollout_knot<64, true, true>(L, Q, h->md, b, kq, eps, o.ReB_active, nullptr, so, s0 + kq, h->fail.data(), true, true, ws, lim);
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
// hsddp_hybrid_rollout with user rows [batch][12], NaN where unset, and scales [batch][84] (null: none set - the LIM programs read ones, the
// lane-quad terminal slots run the program without scales).  user null: with scales pw_emu's entry point; with neither table the launch of a handle
// that has none - the programs without switches, on lane quads where `program` puts them (emu.cpp's own lane-quad switch leaves the terminal knots
// on the one-wave program).  program as in pw_emu_hybrid_rollout.
int lim_emu_hybrid_rollout(hsddp_handle_t* h, double eps, const hsddp_option_t* opt, const double* scales, const double* user, int program) {
    if (user == nullptr && scales != nullptr) return pw_emu_hybrid_rollout(h, eps, opt, scales, program);
    const bool lim_on = user != nullptr;
    OptDev o = to_dev(*opt); SlotOut so{h->cost.data(), h->dsq.data(), h->ming.data(), h->maxh.data()};
    static WbCore L;
    std::vector<PhaseDev> ph = h->ph;
    if (!o.MS) for (auto& q : ph) q.shooting = 0;
    const bool quad = program == 1 && o.MS;
    const std::vector<double> resv = lim_on ? lim_resolve(h, user) : std::vector<double>(), ones((size_t)h->batch * WS_ROW, 1.0);
    struct { const double* p; const double* data() const { return p; } } res{lim_on ? resv.data() : nullptr};
    const double* wtab = scales ? scales : ones.data();
    for (int b = 0; b < h->batch; b++) {
        const double* ws = wtab + (size_t)b * WS_ROW;
        h->fail[b] = 0;
        if (!ph[0].shooting) {
            const int n0 = ph[0].n;
            if (ph[0].model == HSDDP_MODEL_WB) for (int i = 0; i < 36; i++) L.xnext[i] = h->x0[(size_t)b * 36 + i];
            else for (int i = 0; i < n0; i++) ph[0].Xsim[(size_t)b * (ph[0].h + 1) * n0 + i] = h->x0[(size_t)b * n0 + i];
            lim_chain(h, ph, L, 0, b, eps, o, so, ws, res.data());
        } else for (int s = 0; s < h->nslots; s++) {
            int pi = h->sp[s], k = h->sk[s]; const PhaseDev& P = ph[pi]; size_t slot = (size_t)b * h->nslots + s;
            const PhaseDev* Pn = pi + 1 < h->nph ? &ph[pi + 1] : nullptr;
            if (!P.shooting) continue;
            if (P.model == HSDDP_MODEL_HKD) {
                HkdLds& Lh = *reinterpret_cast<HkdLds*>(&L);
                if (k < P.h) hkd_rollout_knot<64>(Lh, P, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data());
                else { hkd_rollout_terminal<64>(Lh, P, Pn, h->md, b, eps, o.AL_active, so, slot); lim_chain(h, ph, L, pi + 1, b, eps, o, so, ws, res.data()); }
            } else if (P.model == HSDDP_MODEL_SRB) {
                SrbLds& Ls = *reinterpret_cast<SrbLds*>(&L);
                if (k < P.h) srb_rollout_knot<64>(Ls, P, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data());
                else { srb_rollout_terminal<64>(Ls, P, Pn, b, eps, so, slot); lim_chain(h, ph, L, pi + 1, b, eps, o, so, ws, res.data()); }
            } else {
                const double gh[4] = {P.ground_height, P.ground_height, P.ground_height, P.ground_height};
                if (!lim_on) {      // no table: the programs without switches
                    if (k < P.h && quad) {
                        const QuadOut q = wbq_rollout_knot<QH>(P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, true);
                        so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = q.ming; so.maxh[slot] = 0.0; if (q.bad) h->fail[b] = 1;
                    } else if (k < P.h) wb_rollout_knot<64>(L, P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data(), false, true);
                    else if (quad && term_owned(h, pi)) {
                        const QuadTermOut q = wbq_rollout_terminal<QH>(P, Pn, h->md, b, eps, o.AL_active, true);
                        so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = 0.0; so.maxh[slot] = q.maxh;
                    } else { wb_rollout_terminal<64>(L, P, Pn, h->md, b, eps, o.AL_active, so, slot, false, true); lim_chain(h, ph, L, pi + 1, b, eps, o, so, ws, nullptr); }
                    continue;
                }
                const double* lim = res.data() + ((size_t)pi * h->batch + b) * LIM_ROW;
                if (k < P.h && quad) {
                    const QuadOut q = wbq_rollout_knot<QH, true, true>(P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, true, ws, lim);
                    so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = q.ming; so.maxh[slot] = 0.0; if (q.bad) h->fail[b] = 1;
                } else if (k < P.h) wb_rollout_knot<64, true, true>(L, P, h->md, b, k, eps, o.ReB_active, pi == 0 ? h->x0.data() : nullptr, so, slot, h->fail.data(), false, true, ws, lim);
                else if (quad && term_owned(h, pi)) {      // terminal knots on lane quads read no limit: the program they run without limits
                    QuadTermOut q;
                    if (scales) q = wbq_rollout_terminal<QH, true, true>(P, Pn, h->md, b, eps, o.AL_active, true, gh, ws);
                    else q = wbq_rollout_terminal<QH>(P, Pn, h->md, b, eps, o.AL_active, true);
                    so.cost[slot] = q.cost; so.dsq[slot] = q.dsq; so.ming[slot] = 0.0; so.maxh[slot] = q.maxh;
                } else { wb_rollout_terminal<64, true, true>(L, P, Pn, h->md, b, eps, o.AL_active, so, slot, false, true, gh, ws); lim_chain(h, ph, L, pi + 1, b, eps, o, so, ws, res.data()); }
            }
        }
        double c = 0, d = 0; for (int s = 0; s < h->nslots; s++) { c += h->cost[(size_t)b * h->nslots + s]; d += h->dsq[(size_t)b * h->nslots + s]; }
        h->acost[b] = c; h->feas[b] = sqrt(d);
    }
    h->cache_valid = true;
    return 0;
}
// hsddp_LQ_approximation with user rows [batch][12] (null: pw_emu's entry point) and scales (null: ones)
int lim_emu_LQ_approximation(hsddp_handle_t* h, const hsddp_option_t* opt, const double* scales, const double* user) {
    if (user == nullptr) return pw_emu_LQ_approximation(h, opt, scales);
    OptDev o = to_dev(*opt); static WbLqLds L; static SrbLds Ls; static HkdLds Lh;
    const std::vector<double> res = lim_resolve(h, user), ones((size_t)h->batch * WS_ROW, 1.0);
    const double* wtab = scales ? scales : ones.data();
    for (int b = 0; b < h->batch; b++) for (int s = 0; s < h->nslots; s++) {
        int pi = h->sp[s], k = h->sk[s]; const PhaseDev& P = h->ph[pi]; const PhaseDev* Pn = pi + 1 < h->nph ? &h->ph[pi + 1] : nullptr;
        const double* ws = wtab + (size_t)b * WS_ROW;
        if (P.model == HSDDP_MODEL_HKD) { if (k < P.h) hkd_lq_knot<EMU_LQ_NT>(Lh, P, b, k, o.ReB_active); else hkd_lq_terminal<EMU_LQ_NT>(Lh, P, Pn, h->md, b, o.AL_active); }
        else if (P.model == HSDDP_MODEL_SRB) { if (k < P.h) srb_lq_knot<EMU_LQ_NT>(Ls, P, b, k, o.ReB_active); else srb_lq_terminal<EMU_LQ_NT>(Ls, P, Pn, b); }
        else if (k < P.h) wb_lq_knot<EMU_LQ_NT, true, true>(L, P, h->md, b, k, o.ReB_active, h->cache_valid, ws, res.data() + ((size_t)pi * h->batch + b) * LIM_ROW);
        else wb_lq_terminal<EMU_LQ_NT, true>(L, P, Pn, h->md, b, o.AL_active, ws);
    }
    return 0;
}
// k_pack_limits' loop on the host (limits.hpp): user [batch][12], res [nph][batch][12], desc [nph][12], the caller's rows [nb][12] for [b0, b0+nb);
// mode 0: first call of hsddp_limits_set, 1: a later call, 2: hsddp_reconfigure (src unread)
int lim_emu_pack(double* user, double* res, const double* desc, int batch, int nph, const double* src, int b0, int nb, int mode) {
    const bool range = mode == hs::LIM_PACK_RANGE;
    hs::lim_pack_host(hs::LimPack{user, res, src, desc, batch, nph, b0, nb, range ? b0 : 0, range ? nb : batch, mode});
    return 0;
}
// k_lim_mu's loop on the host: mu_tab [n_mu][2], mu_of [batch * stride]
int lim_emu_friction(double* user, double* res, int batch, int nph, const double* mu_tab, const int* mu_of, int stride, double kappa) {
    hs::lim_mu_host(hs::LimMu{user, res, mu_tab, mu_of, stride, batch, nph, kappa});
    return 0;
}
// the descriptor rows of the handle's window, [nph][12]
int lim_emu_desc_rows(hsddp_handle_t* h, double* out) { for (int i = 0; i < h->nph; i++) lim_row_of(h->ph[i], out + (size_t)i * LIM_ROW); return h->nph; }
// the argument rules (limits.hpp) as the library applies them
int lim_emu_check_set(int batch, int nph, int f32, int b0, int nb, const double* rows, int src_device) { return hs::lim_check_set(hs::LimHandleInfo{batch, nph, f32}, b0, nb, rows, src_device); }
int lim_emu_check_get(int batch, int nph, int f32, int phase, int b0, int nb) { return hs::lim_check_get(hs::LimHandleInfo{batch, nph, f32}, phase, b0, nb); }
int lim_emu_check_kappa(double kappa) { return hs::lim_check_kappa(kappa); }
}
