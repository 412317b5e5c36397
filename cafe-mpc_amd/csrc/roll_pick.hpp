// Which of the eleven rollout kernels and four LQ kernels a launch uses: the one statement of the rule.  Plain C++ without a HIP header and without the
// handle, so that launch_rollout_list / launch_lq (hsddp_hip.hip) and the stand-alone program of the tests (tests/cpp/roll_pick_table.cpp) share ONE copy.
#pragma once

namespace hs {

// what the dispatch reads.  lim_on / ws_on: a table of per-problem constraint limits / cost-weight scales is in use (hsddp_limits.h, hsddp_weights.h);
// tdh: a phase of the window has touchdown heights of its own (td_n > 0, hsddp_touchdown.h); f32: the handle's precision; has_hkd / has_wb: the window
// has a kinodynamic / a whole-body phase; quad_path: the launch runs its whole-body running knots on lane quads (h->quad && MS && nq > 0); has_term /
// has_other: the quad path owns terminal knots / leaves slots to the one-wave program; has_prob: the launch's problem list is not empty.
struct RollSwitches { bool lim_on, ws_on, tdh, f32, has_hkd, has_wb, quad_path, has_term, has_other, has_prob; };

enum RollKernel {
    RK_NONE,      // the launch does not happen
    RK_ROLLOUT, RK_ROLLOUT_HKD, RK_ROLLOUT_TDH, RK_ROLLOUT_PW, RK_ROLLOUT_LIM,      // one wave per knot
    RK_QUAD, RK_QUAD_PW, RK_QUAD_LIM,                                               // lane quads, running knots
    RK_QUAD_TERM, RK_QUAD_TERM_TDH, RK_QUAD_TERM_PW,                                // lane quads, terminal knots
};
enum LqKernel { LK_LQ, LK_LQ_HKD, LK_LQ_PW, LK_LQ_LIM };
enum RollTier { ROLL_PLAIN, ROLL_PW, ROLL_LIM };      // the timing name's suffix: "", "_pw", "_lim" (roll_suffix)
enum RollWtab { WTAB_NONE, WTAB_HANDLE, WTAB_ONES };  // the scale table the kernels are handed: none, the handle's, the table of 1.0 beside the limits

// quad / term / wave: the up to three launches of a rollout, in this order.  whole_window: the one-wave launch covers every slot and every problem
// (slot_list null, nlist = nslots, unit_knots = nslots - nph, the phases of single shooting when MS is off) - else the slots the quad path leaves it
// and the launch's problem list.  need_tdh: the heights table must be ready first (ws_tdh_ready) - the kernels of both tiers have the heights compiled in.
struct RollPick { RollKernel quad, term, wave; bool whole_window; RollTier tier; bool need_tdh; RollWtab wtab; bool ltab; };
// no_cache: use_cache is 0 whatever the handle's cache says (k_lq_hkd keeps none)
struct LqPick { LqKernel kernel; bool no_cache; RollTier tier; RollWtab wtab; bool ltab; };

// The tier.  Limits and scales act on fp64 handles whose window has a whole-body phase and no kinodynamic one; everything else silently runs the
// plain kernels.  Limits come first: their kernels have the scales compiled in.
inline RollTier roll_tier(const RollSwitches& s) {
    const bool tables = !s.f32 && !s.has_hkd && s.has_wb;
    return tables && s.lim_on ? ROLL_LIM : tables && s.ws_on ? ROLL_PW : ROLL_PLAIN;
}
// limits without scales read ones (x * 1.0 is exact)
inline RollWtab roll_wtab(RollTier t, const RollSwitches& s) { return t == ROLL_PLAIN ? WTAB_NONE : t == ROLL_PW || s.ws_on ? WTAB_HANDLE : WTAB_ONES; }

// The rule.  On the quad path the running knots take the tier's kernel; the terminal knots read no path-constraint limit, so under limits they run what
// they would run without (ws_on alone decides there: the tier's condition already holds) - scaled, else with heights, else plain; the one-wave launch
// takes the slots that are left, if there are any and a problem to run them for (the terminal launch does not ask for a problem).  Off the quad path
// one launch covers the window: the tier's kernel, and in the plain tier the one with heights unless the window has a kinodynamic phase (heights
// exist for whole-body phases only), else the kinodynamic or the whole-body program.  On the quad path has_hkd is not asked again.
inline RollPick roll_pick(const RollSwitches& s) {
    const RollTier t = roll_tier(s);
    RollPick p = {RK_NONE, RK_NONE, RK_NONE, !s.quad_path, t, t != ROLL_PLAIN, roll_wtab(t, s), t == ROLL_LIM};
    if (s.quad_path) {
        p.quad = t == ROLL_LIM ? RK_QUAD_LIM : t == ROLL_PW ? RK_QUAD_PW : RK_QUAD;
        if (s.has_term) p.term = t == ROLL_PW || (t == ROLL_LIM && s.ws_on) ? RK_QUAD_TERM_PW : s.tdh ? RK_QUAD_TERM_TDH : RK_QUAD_TERM;
        if (s.has_other && s.has_prob) p.wave = t == ROLL_LIM ? RK_ROLLOUT_LIM : t == ROLL_PW ? RK_ROLLOUT_PW : s.tdh ? RK_ROLLOUT_TDH : RK_ROLLOUT;
    } else {
        p.wave = t == ROLL_LIM ? RK_ROLLOUT_LIM : t == ROLL_PW ? RK_ROLLOUT_PW : s.tdh && !s.has_hkd ? RK_ROLLOUT_TDH : s.has_hkd ? RK_ROLLOUT_HKD : RK_ROLLOUT;
    }
    return p;
}

// the LQ kernel of the same tier; it is timed as "k_lq" + suffix (k_lq_hkd under k_lq's name) and asks for no heights
inline LqPick lq_pick(const RollSwitches& s) {
    const RollTier t = roll_tier(s);
    const LqKernel k = t == ROLL_LIM ? LK_LQ_LIM : t == ROLL_PW ? LK_LQ_PW : s.has_hkd ? LK_LQ_HKD : LK_LQ;
    return {k, k == LK_LQ_HKD, t, roll_wtab(t, s), t == ROLL_LIM};
}

inline const char* roll_suffix(RollTier t) { return t == ROLL_LIM ? "_lim" : t == ROLL_PW ? "_pw" : ""; }
inline const char* roll_kernel_name(RollKernel k) {
    static const char* const names[] = {"", "k_rollout", "k_rollout_hkd", "k_rollout_tdh", "k_rollout_pw", "k_rollout_lim", "k_rollout_quad", "k_rollout_quad_pw", "k_rollout_quad_lim",
                                        "k_rollout_quad_term", "k_rollout_quad_term_tdh", "k_rollout_quad_term_pw"};
    return names[k];
}
inline const char* roll_kernel_name(LqKernel k) {
    static const char* const names[] = {"k_lq", "k_lq_hkd", "k_lq_pw", "k_lq_lim"};
    return names[k];
}

}  // namespace hs
