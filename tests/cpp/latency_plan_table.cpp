// TEST-ONLY: a stand-alone program around the host rule of the policy latency (cafe-mpc_amd/csrc/latency_plan.hpp: which (phase, knot) a stale step reads
// and which entry of the per-step table the walk is sent to), for -fsanitize=address,undefined.  tests/test_latency_host.py compiles and runs it.  Every
// map lives in a heap block of exactly the size the rule is documented to write, so that a step too many is an error of the sanitizer.  Prints
// "latency_plan_table: clean" when every case answered as expected.
#include <cstdio>
#include <vector>
#include "latency_plan.hpp"

using namespace hs;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("latency_plan_table: " __VA_ARGS__); std::printf(" [%s]\n", #cond); failures++; } } while (0)

struct Plan { bool ok; int pending; std::vector<int> lm, wm; };
static Plan plan(const std::vector<LatPhase>& ph, int n_exec, int D) {
    Plan p;
    p.lm.assign(3 * (size_t)(n_exec + D), -7); p.wm.assign(3 * (size_t)n_exec, -7); p.pending = -9;
    p.ok = lat_plan(ph.data(), (int)ph.size(), n_exec, D, p.lm.data(), p.wm.data(), &p.pending);
    return p;
}
// the checks every accepted plan has to pass: consecutive knots, rows inside their phase, the walk map naming entry s
static void check_common(const char* tag, const std::vector<LatPhase>& ph, int n_exec, int D, const Plan& p) {
    const int L = n_exec + D;
    for (int s = 0; s < L; s++) {
        const int pi = p.lm[s], k = p.lm[L + s];
        EXPECT(pi >= 0 && pi < (int)ph.size() && ph[pi].wb, "%s: step %d names phase %d", tag, s, pi);
        EXPECT(k >= 0 && k < ph[pi].h, "%s: step %d reads Ubar / K row %d of %d", tag, s, k, ph[pi].h);
        EXPECT(k + 1 <= ph[pi].h, "%s: step %d reads Xbar row %d of %d", tag, s, k + 1, ph[pi].h + 1);      // the terminal knot at most
        if (s > 0) {
            const int pp = p.lm[s - 1], kp = p.lm[L + s - 1];
            EXPECT((pi == pp && k == kp + 1) || (pi == pp + 1 && k == 0 && kp == ph[pp].h - 1), "%s: step %d does not follow step %d", tag, s, s - 1);
        }
        const bool td = k == ph[pi].h - 1 && ph[pi].has_impact;
        EXPECT(p.lm[2 * L + s] == ((td && s + 1 < L) ? 1 : 0), "%s: reset flag of step %d of the long map", tag, s);
    }
    for (int s = 0; s < n_exec; s++) {
        const int pi = p.lm[s], k = p.lm[L + s];
        const bool td = k == ph[pi].h - 1 && ph[pi].has_impact;
        EXPECT(p.wm[s] == s && p.wm[n_exec + s] == 0, "%s: the walk map sends step %d to entry %d knot %d", tag, s, p.wm[s], p.wm[n_exec + s]);
        EXPECT(p.wm[2 * n_exec + s] == ((td && s + 1 < n_exec) ? 1 : 0), "%s: reset flag of step %d of the walk map", tag, s);
    }
}

int main() {
    const LatPhase wb3i = {1, 3, 1}, wb4 = {1, 4, 0}, wb2i = {1, 2, 1}, srb = {0, 5, 0};
    {   // a stale step on a phase's last knot: the row behind it is the terminal knot
        const std::vector<LatPhase> ph = {wb3i, wb4, srb};
        const Plan p = plan(ph, 2, 1);
        EXPECT(p.ok, "last knot: refused");
        if (p.ok) {
            check_common("last knot", ph, 2, 1, p);
            EXPECT(p.lm[2] == 0 && p.lm[3 + 2] == 2, "last knot: stash row 0 reads (%d, %d)", p.lm[2], p.lm[3 + 2]);
            EXPECT(p.lm[3 + 2] + 1 == ph[0].h, "last knot: the next row is not the terminal knot");
            EXPECT(p.pending == -1, "last knot: pending %d", p.pending);
        }
    }
    {   // stale steps on both sides of a phase boundary with a reset map; D = n_exec
        const std::vector<LatPhase> ph = {wb3i, wb4, srb};
        const Plan p = plan(ph, 2, 2);
        EXPECT(p.ok, "straddle: refused");
        if (p.ok) {
            check_common("straddle", ph, 2, 2, p);
            EXPECT(p.lm[2] == 0 && p.lm[4 + 2] == 2 && p.lm[3] == 1 && p.lm[4 + 3] == 0, "straddle: stash rows read (%d, %d) (%d, %d)", p.lm[2], p.lm[4 + 2], p.lm[3], p.lm[4 + 3]);
            EXPECT(p.lm[8 + 2] == 1, "straddle: the reset map behind step 2 is not in the long map");
            EXPECT(p.wm[4] == 0 && p.wm[5] == 0, "straddle: the walk map has a reset inside the tick");
        }
    }
    {   // the tick ends on the touchdown: the pending map is not the walk's, and the long map has it
        const std::vector<LatPhase> ph = {wb3i, wb4, srb};
        const Plan p = plan(ph, 3, 3);
        EXPECT(p.ok, "pending: refused");
        if (p.ok) {
            check_common("pending", ph, 3, 3, p);
            EXPECT(p.pending == 0, "pending: %d", p.pending);
            EXPECT(p.wm[6 + 2] == 0 && p.lm[12 + 2] == 1, "pending: reset flags of step 2: walk %d long %d", p.wm[6 + 2], p.lm[12 + 2]);
        }
    }
    {   // a reset inside the tick, and two short phases inside the stash
        const std::vector<LatPhase> ph = {wb2i, wb2i, wb2i, srb};
        const Plan p = plan(ph, 3, 3);
        EXPECT(p.ok, "short phases: refused");
        if (p.ok) {
            check_common("short phases", ph, 3, 3, p);
            EXPECT(p.wm[6 + 1] == 1 && p.pending == -1, "short phases: walk reset %d pending %d", p.wm[6 + 1], p.pending);
            EXPECT(p.lm[18 - 1] == 0, "short phases: a reset behind the last step of the long map");
        }
    }
    {   // a window one knot too short is refused; the same window with one stale step less is accepted; D = 0 is the plain map
        const std::vector<LatPhase> ph = {wb3i, wb4, srb};      // seven whole-body knots
        EXPECT(!plan(ph, 4, 4).ok, "too short: n_exec 4 + D 4 accepted on 7 knots");
        EXPECT(plan(ph, 4, 3).ok, "too short: n_exec 4 + D 3 refused on 7 knots");
        EXPECT(!plan({wb3i, srb, wb4}, 2, 2).ok, "too short: knots behind the single-rigid-body phase were counted");
        const Plan p = plan(ph, 4, 0);
        EXPECT(p.ok, "D = 0: refused");
        if (p.ok) check_common("D = 0", ph, 4, 0, p);
    }
    EXPECT(lat_is_stale(0, 1, true) && !lat_is_stale(1, 1, true) && !lat_is_stale(0, 1, false) && !lat_is_stale(0, 0, true), "lat_is_stale");
    EXPECT(LAT_ROW == 36 + 36 + 12 + 432 && LAT_OU == 72 && LAT_OK == 84, "the row layout");
    if (failures == 0) std::printf("latency_plan_table: clean\n");
    return failures == 0 ? 0 : 1;
}
