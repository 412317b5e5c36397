/*
 * hsddp_latency.h — per-robot policy latency in the closed-loop MPC episodes of include/hsddp_episode.h (libhsddp_hip.so).
 *
 * Without it a tick applies the policy the handle holds from its first step on: the solve takes no time.  With it robot b has a delay d_b, in
 * CONTROL steps, 0 <= d_b <= n_exec.  In tick t >= 1 the steps s < d_b apply the PREVIOUS policy - the one the handle held during tick t - 1, at
 * knots n_exec + s of that window, the same physical time - and the steps s >= d_b apply the handle's current policy at knot s.
 *
 * The policy row of a step is Xbar[k] | Xbar[k+1] | Ubar[k] | K[k]: 36 + 36 + 12 + 432 = 516 doubles.  Xbar[k+1] is the knot that follows in the
 * same phase (the terminal knot included); the walk measures the deviation of the state behind the last step against it.  K is column-major
 * 12 x 36, the handle's order.
 *
 * Only the policy is stale.  The solve still starts from the state measured at the start of the tick, and the contact schedule, dt, the reset
 * maps, the pending impact, and the weights and references of the commit all come from the current window.
 *
 *   - Tick 0 after a reset runs fresh, and so does the first tick after latency is switched on: stale rows are used only when the previous
 *     hsddp_episode_advance since the last reset ran with latency on and left a stash.
 *   - dev_q and dev_v of a tick (hsddp_episode_row_t) are deviations from the EFFECTIVE plan: from the stale Xbar rows on stale steps.
 *   - A frozen robot is composed like every other one (its walk still runs and is ignored); its n_stale no longer grows.
 *   - The window MUST move by exactly n_exec knots between two ticks, as in the loop of hsddp_episode.h: knot n_exec + s of the previous window
 *     and knot s of the current one are then the same physical time.  The library cannot check this.
 *
 * Out of scope: delay compensation by planning from a predicted state; delays longer than one tick; delays at sub-step granularity (the walk
 * fetches a policy row once per control step, so a delay counts control steps whatever hsddp_substep_set says).
 *
 * hsddp_latency_set allocates everything, with D the largest delay: the effective policy [B][n_exec][516], two stashes [B][D][516] used in
 * turn (one is read while the other is written), the per-step descriptor table and step map the walk is launched on, the delays and the
 * counters.  A later call with a larger D allocates the stashes again.  hsddp_episode_advance and hsddp_episode_reset still allocate nothing
 * (hsddp_debug_malloc_count), also across hsddp_reconfigure.  The call invalidates the stash and keeps n_stale.  on = 0 switches latency off:
 * hsddp_episode_advance then launches exactly what it launched before this header existed.
 *
 * hsddp_episode_advance with latency on launches ONE more kernel, k_episode_latency, behind the rebind of the step map and in front of the
 * walk (timed into the handle's kernel table, hsddp_get_kernel_times): it composes the effective row of every (robot, step), writes the next
 * stash from the handle's knots n_exec .. n_exec + D - 1 and counts n_stale.  The walk then reads the effective rows; the commit and the
 * pending impact read the handle as before.  The current window has to lead with n_exec + D whole-body knots; otherwise HSDDP_EINVAL with
 * nothing changed (states, rows, log, tick, the handle, the stash).
 *
 * hsddp_episode_reset invalidates the stash and zeroes n_stale; it keeps the delays.
 *
 * HSDDP_EINVAL with nothing changed: a NULL episode, a delay outside [0, n_exec], a NULL destination of hsddp_latency_get, [b0, b0+nb) outside the
 * batch, hsddp_latency_get before the first hsddp_latency_set, hsddp_latency_get_policy before any tick ran with latency on.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_LATENCY_H
#define HSDDP_LATENCY_H
#include "hsddp_episode.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_latency_row { int delay, n_stale; } hsddp_latency_row_t;   /* n_stale: stale steps executed while alive since the reset */

int hsddp_latency_set(hsddp_episode_t *e, int on, const int *delay_of /* [B] host, or NULL */, int delay /* for all when delay_of is NULL */);
int hsddp_latency_get(hsddp_episode_t *e, int b0, int nb, hsddp_latency_row_t *rows);
/* the effective policy the LAST tick walked, problems [b0, b0+nb): Xe [nb][n_exec][2][36], Ue [nb][n_exec][12], Ke [nb][n_exec][432]; NULL skips one */
int hsddp_latency_get_policy(hsddp_episode_t *e, int b0, int nb, double *Xe, double *Ue, double *Ke);

#ifdef __cplusplus
}
#endif
#endif
