// Policy latency of the MPC episodes (include/hsddp_latency.h): which (phase, knot) of the window a step reads its policy row from, and which entry
// of the per-step descriptor table the walk is sent to.  Plain C++ without a HIP header, so that hsddp_episode_advance (sim_host.hpp) and the
// stand-alone program of the tests (tests/cpp/latency_plan_table.cpp) share ONE copy of the rule.
#pragma once

namespace hs {

constexpr int LAT_ROW = 516;      // doubles of a policy row: Xbar[k] (36) | Xbar[k+1] (36) | Ubar[k] (12) | K[k] (432, column-major 12 x 36)
constexpr int LAT_OX = 0, LAT_OU = 72, LAT_OK = 84;      // offsets of the three parts in a stashed row

struct LatPhase { int wb, h, has_impact; };      // what the rule needs of a phase of the window: whole-body or not, control knots, a touchdown behind the last

// The plan of a tick with n_exec executed steps and largest delay D over the window ph[0 .. nph):
//   long_map  [3][n_exec + D]  step -> phase, knot, reset map behind the step, over the n_exec + D leading whole-body control knots, as the
//             simulation object's map over that many steps.  Step s < n_exec of it is the fresh source of step s; step n_exec + j is what stash row j
//             is read from - and what STALE step j of the NEXT tick applies, once the window has moved by n_exec knots.  The row of (phase p, knot k)
//             is Xbar rows k and k + 1 of p (k + 1 <= h: the terminal knot when k is the phase's last), Ubar row k, K row k.
//   walk_map  [3][n_exec]      what the walk gets instead of the real map: (s, 0, reset of step s) - entry s of a table of n_exec descriptors with
//             h = 1, whose policy pointers lead to the composed rows of step s.  reset is the flag of the map over n_exec steps: nothing behind the
//             last step (that map is the pending impact's).
//   pending   the phase whose reset map lies behind step n_exec - 1, else -1.
// False, with nothing written that matters, if the window leads with fewer than n_exec + D whole-body control knots.
inline bool lat_plan(const LatPhase* ph, int nph, int n_exec, int D, int* long_map, int* walk_map, int* pending) {
    const int L = n_exec + D;
    int n = 0, pend = -1;
    for (int i = 0; i < nph && n < L; i++) {
        if (!ph[i].wb) break;
        for (int k = 0; k < ph[i].h && n < L; k++, n++) {
            const bool td = k == ph[i].h - 1 && ph[i].has_impact != 0;
            long_map[n] = i; long_map[L + n] = k; long_map[2 * L + n] = (td && n + 1 < L) ? 1 : 0;
            if (n < n_exec) {
                walk_map[n] = n; walk_map[n_exec + n] = 0; walk_map[2 * n_exec + n] = (td && n + 1 < n_exec) ? 1 : 0;
                if (td && n + 1 == n_exec) pend = i;
            }
        }
    }
    if (pending) *pending = pend;
    return n == L;
}

// which steps of a tick are stale for a robot with delay d: s < d, and only with a stash from the previous tick
inline bool lat_is_stale(int s, int d, bool stash_valid) { return stash_valid && s < d; }

}  // namespace hs
