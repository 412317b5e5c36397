/*
 * hsddp_substep.h — sub-stepped integration of a closed-loop simulation object (include/hsddp_sim.h, include/hsddp_mc.h, include/hsddp_grf.h,
 * include/hsddp_episode.h; libhsddp_hip.so).
 *
 * A simulation advances the robot with the step the planner assumed: one forward-Euler step of the phase's dt per control knot.  The simulated
 * plant is then the planner's own discretisation.  With substeps = S > 1 every control knot is split into S forward-Euler steps of dt / S under
 * the knot's torque (zero-order hold): a finer integrator under the same policy.  The setting belongs to the object, like hsddp_grf_set, and
 * holds for every later hsddp_sim_run and hsddp_mc_run of it.
 *
 * Step s of a live sample (phase i, knot k) with S substeps:
 *   1. Everything hsddp_sim.h / hsddp_mc.h do at the head of a step, unchanged and ONCE per control step: the push (s == kick_step); the record
 *      of x (dev_q, dev_v, min_height, trajectory entry s); the fall test; the noise of step s - the generator numbers its draws by (seed,
 *      problem, sample, CONTROL step, coordinate), so a run with S substeps draws the normals of the run with one; u_cmd, actuator noise, n_sat,
 *      the clip, max_torque, U[s].
 *   2. h = dt / S (one IEEE double division), then for j = 0 .. S-1:  x <- x + h (v, qdd(x, u))  with the contact dynamics of phase i, the SAME
 *      u, the phase's Baumgarte bg_alpha and Gram damping 1e-12.
 *   3. The divergence test (hsddp_sim.h) runs on the new state after EVERY substep.  A failing substep sets first_bad = s; the sample keeps the
 *      state it had before that substep through the remaining substeps and all later steps, and records nothing further.  (Its lane quad still
 *      executes them, as a diverged sample's does without substeps: the cost of a run does not depend on which samples diverge.)
 *   4. The reset map of a phase comes behind the last substep of its last knot, as without substeps.
 *
 * State records exist at control instants only: rows, X, U, x_final and the extras keep their shapes and meanings.
 *
 * Force records (hsddp_grf_set on):
 *   - min_fz, min_cone and max_fz run over every substep of every stance foot; a substep counts if the sample was alive when it began.
 *   - first_slip is the CONTROL step of the first violating substep.
 *   - n_slip counts violating (foot, SUBSTEP) pairs: with S substeps a foot that violates through a whole control step adds S, not 1.  n_slip / S
 *     is the count in control-step equivalents.
 *   - Y[b][r][s] is the force of substep 0 of step s: the force at the state the control is applied from, as without substeps.
 *   sim.grf_rows_sub states these rules in numpy.
 *
 * Rules:
 *   - hsddp_substep_set(s, S), 1 <= S <= HSDDP_SUBSTEP_MAX.  HSDDP_EINVAL with nothing changed: S outside that range, a NULL argument.
 *   - S = 1 (and an object on which the call was never made) launches exactly the kernels hsddp_sim.h, hsddp_mc.h and hsddp_grf.h launch: a run is
 *     bit-identical to one before this header existed.
 *   - The first call with S > 1 allocates one small block of device memory; later calls and all runs allocate nothing
 *     (hsddp_debug_malloc_count).  The handle is left bit for bit as it was, as by every simulation call.
 *   - hsddp_substep_get returns what later runs use (1 on a fresh object).
 *   - Episodes: hsddp_episode_sim(e) may be passed to hsddp_substep_set and hsddp_substep_get as well as to hsddp_grf_set.  The setting is the
 *     internal simulation object's and survives the rebind of its step map after hsddp_reconfigure.  Commit, tracking cost, log and hand-off are
 *     unchanged: they read control instants.  The pending impact of an episode (k_episode_impact) is not sub-stepped - it is a map, not a step.
 *
 * Out of scope: re-evaluating the feedback inside a knot (the torque is held); integrators of higher order; fp32 handles and windows that do not
 * lead with whole-body knots (hsddp_sim_create refuses those already).
 */
#ifndef HSDDP_SUBSTEP_H
#define HSDDP_SUBSTEP_H
#include "hsddp_sim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HSDDP_SUBSTEP_MAX 64

int hsddp_substep_set(hsddp_sim_t *s, int substeps);        /* 1 <= substeps <= HSDDP_SUBSTEP_MAX */
int hsddp_substep_get(hsddp_sim_t *s, int *substeps);       /* what later runs use (1 on a fresh object) */

#ifdef __cplusplus
}
#endif
#endif
