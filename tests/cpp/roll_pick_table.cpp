// TEST-ONLY: a stand-alone program around the dispatch rule of the solver's rollout and LQ launches (cafe-mpc_amd/csrc/roll_pick.hpp: which of the eleven
// rollout kernels and four LQ kernels a launch uses, under which timing name, with which tables), for -fsanitize=address,undefined.
// tests/test_limits_host.py compiles and runs it.  It walks all 2^10 switch settings and compares roll_pick / lq_pick field by field with expected() below:
// a LITERAL transcription of the nested branches launch_rollout_list, launch_rollout_lim, launch_lq, ws_table, lim_table and lim_wtab had before the rule
// was written down in one place (same order of tests, same early exits) - the reference, not the rule rephrased.  It then checks that exactly the fifteen
// kernels are reachable, that handles without tables and heights launch the six kernels of before, that the documented inert combinations are inert and
// that the timing suffix follows the kernel, and prints "roll_pick_table: clean" when everything answered as expected.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include "roll_pick.hpp"

using namespace hs;

static int failures = 0;
static void fail(const RollSwitches& s, const char* what, const std::string& got, const std::string& want) {
    std::printf("roll_pick_table: lim %d ws %d tdh %d f32 %d hkd %d wb %d quad %d term %d other %d prob %d: %s: got %s, want %s\n", (int)s.lim_on, (int)s.ws_on, (int)s.tdh, (int)s.f32,
                (int)s.has_hkd, (int)s.has_wb, (int)s.quad_path, (int)s.has_term, (int)s.has_other, (int)s.has_prob, what, got.c_str(), want.c_str());
    failures++;
}

// what a launch did before: kernel names ("" = no launch), the form of the one-wave launch, the name it was timed under (suffix), whether ws_tdh_ready
// was asked first, the scale table ("none", "handle": d_ws, "ones": d_lim + lim_off_ones) and whether the resolved limits were passed
struct Want { std::string quad, term, wave; bool whole_window; std::string suffix; bool need_tdh; std::string wtab; bool ltab; std::string lq; bool lq_no_cache; std::string lq_suffix, lq_wtab; bool lq_ltab; };

static bool had_ws_table(const RollSwitches& s) {
    if (!s.ws_on || s.f32 || s.has_hkd) return false;
    if (s.has_wb) return true;      // for (P : h->ph) if (P.model == HSDDP_MODEL_WB) return h->d_ws;
    return false;
}
static bool had_lim_table(const RollSwitches& s) {
    if (!s.lim_on || s.f32 || s.has_hkd) return false;
    if (s.has_wb) return true;
    return false;
}
static std::string had_lim_wtab(const RollSwitches& s) { return s.ws_on ? "handle" : "ones"; }

static void had_rollout_lim(const RollSwitches& s, Want& w) {
    w.need_tdh = true;      // if (ws_tdh_ready(h) != HSDDP_OK) { ...; return; }
    w.wtab = had_lim_wtab(s); w.ltab = true;
    w.suffix = "_lim";
    if (s.quad_path) {
        w.quad = "k_rollout_quad_lim";
        if (s.has_term && s.ws_on) w.term = "k_rollout_quad_term_pw";
        else if (s.has_term && s.tdh) w.term = "k_rollout_quad_term_tdh";
        else if (s.has_term) w.term = "k_rollout_quad_term";
        if (s.has_other && s.has_prob) w.wave = "k_rollout_lim";
        return;
    }
    w.wave = "k_rollout_lim"; w.whole_window = true;
}
static void had_rollout_list(const RollSwitches& s, Want& w) {
    w.whole_window = false; w.need_tdh = false; w.wtab = "none"; w.ltab = false;
    if (had_lim_table(s)) { had_rollout_lim(s, w); return; }
    const bool wtab = had_ws_table(s);
    if (wtab) { w.need_tdh = true; w.wtab = "handle"; }      // if (wtab && ws_tdh_ready(h) != HSDDP_OK) { ...; return; }
    w.suffix = wtab ? "_pw" : "";
    if (s.quad_path) {
        if (wtab) {
            w.quad = "k_rollout_quad_pw";
            if (s.has_term) w.term = "k_rollout_quad_term_pw";
            if (s.has_other && s.has_prob) w.wave = "k_rollout_pw";
            return;
        }
        w.quad = "k_rollout_quad";
        const bool tdh = s.tdh;
        if (s.has_term && tdh) w.term = "k_rollout_quad_term_tdh";
        else if (s.has_term) w.term = "k_rollout_quad_term";
        if (s.has_other && s.has_prob && tdh) w.wave = "k_rollout_tdh";
        else if (s.has_other && s.has_prob) w.wave = "k_rollout";
        return;
    }
    w.whole_window = true;
    if (wtab) { w.wave = "k_rollout_pw"; return; }
    if (s.tdh && !s.has_hkd) { w.wave = "k_rollout_tdh"; return; }
    w.wave = s.has_hkd ? "k_rollout_hkd" : "k_rollout";
}
static void had_lq(const RollSwitches& s, Want& w) {
    w.lq_no_cache = false; w.lq_wtab = "none"; w.lq_ltab = false;
    if (had_lim_table(s)) { w.lq_suffix = "_lim"; w.lq = "k_lq_lim"; w.lq_wtab = had_lim_wtab(s); w.lq_ltab = true; return; }
    if (had_ws_table(s)) { w.lq_suffix = "_pw"; w.lq = "k_lq_pw"; w.lq_wtab = "handle"; return; }
    w.lq_suffix = "";      // Timed t(h, "k_lq") for both
    if (s.has_hkd) { w.lq = "k_lq_hkd"; w.lq_no_cache = true; }
    else w.lq = "k_lq";
}
static Want expected(const RollSwitches& s) { Want w; had_rollout_list(s, w); had_lq(s, w); return w; }

static const char* wtab_name(RollWtab t) { return t == WTAB_HANDLE ? "handle" : t == WTAB_ONES ? "ones" : "none"; }
static const char* yn(bool b) { return b ? "yes" : "no"; }
static bool same(const RollPick& a, const RollPick& b) {
    return a.quad == b.quad && a.term == b.term && a.wave == b.wave && a.whole_window == b.whole_window && a.tier == b.tier && a.need_tdh == b.need_tdh && a.wtab == b.wtab && a.ltab == b.ltab;
}
static bool same(const LqPick& a, const LqPick& b) { return a.kernel == b.kernel && a.no_cache == b.no_cache && a.tier == b.tier && a.wtab == b.wtab && a.ltab == b.ltab; }
static bool ends_with(const std::string& n, const char* tail) { const size_t k = std::strlen(tail); return n.size() >= k && n.compare(n.size() - k, k, tail) == 0; }
static std::string suffix_of(const std::string& kernel) { return ends_with(kernel, "_lim") ? "_lim" : ends_with(kernel, "_pw") ? "_pw" : ""; }

int main() {
    const std::set<std::string> rollouts = {"k_rollout", "k_rollout_hkd", "k_rollout_tdh", "k_rollout_pw", "k_rollout_lim", "k_rollout_quad", "k_rollout_quad_pw", "k_rollout_quad_lim",
                                            "k_rollout_quad_term", "k_rollout_quad_term_tdh", "k_rollout_quad_term_pw"};
    const std::set<std::string> lqs = {"k_lq", "k_lq_hkd", "k_lq_pw", "k_lq_lim"};
    const std::set<std::string> before = {"k_rollout", "k_rollout_hkd", "k_rollout_quad", "k_rollout_quad_term", "k_lq", "k_lq_hkd"};      // what a handle without tables and heights launches
    std::set<std::string> reached_roll, reached_lq;
    int settings = 0;
    for (int bits = 0; bits < 1024; bits++, settings++) {
        const RollSwitches s = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0, (bits & 128) != 0, (bits & 256) != 0,
                                (bits & 512) != 0};
        const RollPick p = roll_pick(s);
        const LqPick q = lq_pick(s);
        const Want w = expected(s);
        const std::string quad = roll_kernel_name(p.quad), term = roll_kernel_name(p.term), wave = roll_kernel_name(p.wave), lq = roll_kernel_name(q.kernel);
        // 1. field by field against the transcription
        if (quad != w.quad) fail(s, "the quad running kernel", quad, w.quad);
        if (term != w.term) fail(s, "the quad terminal kernel", term, w.term);
        if (wave != w.wave) fail(s, "the one-wave kernel", wave, w.wave);
        if (p.whole_window != w.whole_window) fail(s, "one-wave launch over the whole window", yn(p.whole_window), yn(w.whole_window));
        if (w.suffix != roll_suffix(p.tier)) fail(s, "the timing suffix", roll_suffix(p.tier), w.suffix);
        if (p.need_tdh != w.need_tdh) fail(s, "the height table asked for first", yn(p.need_tdh), yn(w.need_tdh));
        if (w.wtab != wtab_name(p.wtab)) fail(s, "the scale table", wtab_name(p.wtab), w.wtab);
        if (p.ltab != w.ltab) fail(s, "the limits passed", yn(p.ltab), yn(w.ltab));
        if (lq != w.lq) fail(s, "the LQ kernel", lq, w.lq);
        if (q.no_cache != w.lq_no_cache) fail(s, "the LQ cache forced off", yn(q.no_cache), yn(w.lq_no_cache));
        if (w.lq_suffix != roll_suffix(q.tier)) fail(s, "the LQ timing suffix", roll_suffix(q.tier), w.lq_suffix);
        if (w.lq_wtab != wtab_name(q.wtab)) fail(s, "the LQ scale table", wtab_name(q.wtab), w.lq_wtab);
        if (q.ltab != w.lq_ltab) fail(s, "the LQ limits passed", yn(q.ltab), yn(w.lq_ltab));
        // 2. only the fifteen
        for (const std::string& k : {quad, term, wave}) if (!k.empty()) { if (!rollouts.count(k)) fail(s, "a rollout kernel of the library", k, "one of the eleven"); reached_roll.insert(k); }
        if (!lqs.count(lq)) fail(s, "an LQ kernel of the library", lq, "one of the four");
        reached_lq.insert(lq);
        if (quad.empty() != !s.quad_path) fail(s, "a quad running launch exactly on the quad path", quad, s.quad_path ? "a kernel" : "none");
        if (!s.quad_path && (wave.empty() || !term.empty())) fail(s, "one launch off the quad path", wave + "|" + term, "a one-wave kernel alone");
        // 3. no tables, no heights: the kernels of before, under the names of before, nothing asked of the height table
        if (!s.lim_on && !s.ws_on && !s.tdh) {
            for (const std::string& k : {quad, term, wave, lq}) if (!k.empty() && !before.count(k)) fail(s, "without tables and heights", k, "one of the six kernels of before");
            if (p.tier != ROLL_PLAIN || q.tier != ROLL_PLAIN) fail(s, "without tables and heights, the suffix", std::string(roll_suffix(p.tier)) + "|" + roll_suffix(q.tier), "none");
            if (p.need_tdh) fail(s, "without tables and heights, the height table asked for", "yes", "no");
        }
        // 4. fp32 handles and windows with a kinodynamic phase or without a whole-body one: limits and scales are inert
        if (s.f32 || s.has_hkd || !s.has_wb) for (int flip = 1; flip < 4; flip++) {
            RollSwitches t = s; if (flip & 1) t.lim_on = !s.lim_on; if (flip & 2) t.ws_on = !s.ws_on;
            if (!same(p, roll_pick(t))) fail(s, "limits / scales where they do not act (rollout)", roll_kernel_name(roll_pick(t).wave), wave);
            if (!same(q, lq_pick(t))) fail(s, "limits / scales where they do not act (LQ)", roll_kernel_name(lq_pick(t).kernel), lq);
        }
        // 5. the launch is timed under the suffix of its quad running kernel, or of its one-wave kernel; where both are launched they agree
        const std::string lead = s.quad_path ? quad : wave;
        if (suffix_of(lead) != roll_suffix(p.tier)) fail(s, "the timing suffix against the leading kernel's", roll_suffix(p.tier), lead + ": " + suffix_of(lead));
        if (s.quad_path && !wave.empty() && suffix_of(wave) != suffix_of(quad)) fail(s, "quad and one-wave kernel of one tier", wave, quad);
        if (suffix_of(lq) != roll_suffix(q.tier)) fail(s, "the suffix of the LQ kernel", roll_suffix(q.tier), suffix_of(lq));
    }
    if (settings != 1024) { std::printf("roll_pick_table: %d settings walked, want 1024\n", settings); failures++; }
    for (const std::string& k : rollouts) if (!reached_roll.count(k)) { std::printf("roll_pick_table: %s is never launched\n", k.c_str()); failures++; }
    for (const std::string& k : lqs) if (!reached_lq.count(k)) { std::printf("roll_pick_table: %s is never launched\n", k.c_str()); failures++; }
    if (reached_roll.size() != 11 || reached_lq.size() != 4) { std::printf("roll_pick_table: %zu + %zu kernels reached, want 11 + 4\n", reached_roll.size(), reached_lq.size()); failures++; }
    if (failures == 0) std::printf("roll_pick_table: clean\n");
    return failures == 0 ? 0 : 1;
}
