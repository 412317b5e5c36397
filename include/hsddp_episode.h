/*
 * hsddp_episode.h — batched closed-loop MPC episodes with the state handed from the simulation to the next solve on the device, on top of
 * include/hsddp_sim.h, include/hsddp_mc.h and include/hsddp_grf.h (libhsddp_hip.so).
 *
 * An episode is B robots, one per problem of the handle, each running its own MPC against the simulated whole-body dynamics for up to
 * max_ticks ticks.  A tick executes the first n_exec control knots of the policy the handle holds, from the episode's own states, and leaves
 * the states it reaches in the handle's initial condition; the caller then moves the window by n_exec knots (hsddp_reconfigure), optionally
 * gives new references (hsddp_set_references) and solves again - the loop of MHPCLocomotion::update, and of testTrajOptInLoop.cpp with the
 * simulated state fed back instead of the plan's own:
 *
 *     hsddp_episode_reset(e, x0, 0);  hsddp_solve(h, ...);
 *     for every tick:  hsddp_episode_advance(e, dist, kick, 0);  hsddp_reconfigure(h, <window moved by n_exec knots>);  hsddp_solve(h, ...);
 *
 * The object owns the states [B][36] on the device, an internal simulation object (one sample per problem, n_exec steps, trajectories kept),
 * one row per problem and, with keep_log, the log: X [B][max_ticks n_exec + 1][36], U [B][max_ticks n_exec][12] and Y (forces) of the shape
 * of U.  hsddp_episode_create allocates all of it; hsddp_episode_advance and hsddp_episode_reset allocate nothing
 * (hsddp_debug_malloc_count), also across hsddp_reconfigure - except the buffers the first disturbed run and the first hsddp_grf_set of the
 * internal simulation object allocate at their first use, as for every simulation object.
 *
 * hsddp_episode_reset   sets the states, empties the rows and zeroes the log, sets tick = 0 and the impact count to 0, and writes the states
 *                       into the handle's initial condition (the effect of hsddp_set_initial_condition for every problem).  x0: [B][36], host
 *                       memory (src_device = 0) or device memory on the handle's device (1).  An empty row is all zero except what a running
 *                       minimum or maximum starts from and the step indices: min_height, min_fz, min_cone = +inf, max_fz = -inf, first_slip =
 *                       end_step = -1.
 *
 * hsddp_episode_advance is tick t = the number of ticks advanced since the last reset:
 *   1. If hsddp_reconfigure moved the window since the object last looked, the step map of the internal simulation object is computed again on
 *      the host and copied (3 n_exec ints; no allocation).  The object never goes stale.
 *   2. HSDDP_EINVAL with nothing changed (states, rows, log, tick, the handle): the first n_exec control knots of the window are not all
 *      whole-body knots; an fp32 handle (refused by hsddp_episode_create already); t == max_ticks; a disturbance hsddp_mc_run refuses (a negative
 *      or non-finite sigma, a non-finite u_max or fall_height, first_problem < 0, kick_step outside [0, n_exec) when a kick is given); a kick
 *      without a dist (the step of the push is the disturbance's); a NULL object; no hsddp_episode_reset yet.
 *   3. The walk: hsddp_sim_run (dist NULL, or everything in it off and no kick) or hsddp_mc_run from the episode's states over n_exec steps,
 *      with the kernels those calls launch - the twins with contact-force records after hsddp_grf_set(hsddp_episode_sim(e), ...).  The noise
 *      of tick t uses the seed tick_seed(dist->seed, t): tick_seed(seed, 0) = seed, and for t >= 1 the t-th raw 64-bit output of
 *      SplitMix64(seed) (hsddp_mc.h: state seed + t 0x9E3779B97F4A7C15 mod 2^64, two multiply-xorshift rounds, before the shift by 11).  A
 *      one-tick episode is hsddp_mc_run bit for bit.  kick_step counts from the tick's first step; kick is [B][36] (host or device).
 *      first_problem is passed through: a shard reproduces its slice.
 *   4. The commit (kernel k_episode_commit), for every problem that was alive at the start of the tick:
 *        log    entries t n_exec .. (t+1) n_exec of X, t n_exec .. (t+1) n_exec - 1 of U and Y are the tick's trajectory (hsddp_sim.h: entry j is
 *               the state control j is applied from, the last the tick's final state).  The next tick writes its own entry 0 over entry
 *               (t+1) n_exec: the same state unless a reset map or a push at step 0 lies between.
 *        row    dev_q, dev_v, max_torque, max_fz: running maxima; min_height, min_fz, min_cone: running minima; n_sat, n_slip: sums;
 *               first_slip: the first violating step as a global step index (t n_exec + step), else -1; steps += n_exec; bad_solves += 1 if the
 *               handle's last solve left status 1 for the problem; track_cost += the realised tracking cost of the tick,
 *                   sum over the tick's steps s of  1/2 sum_i q_i (x_s,i - xr_s,i)^2 + 1/2 sum_j r_j (u_s,j - ur_s,j)^2
 *               with x_s the state control s is applied from, u_s the applied control, q and r the weights of the phase step s maps to, and
 *               xr, ur the reference row of that knot - the problem's own where hsddp_set_references gave it one.  Without a disturbed run
 *               n_sat adds 0; without the force records min_fz, min_cone, max_fz, first_slip, n_slip are left alone.
 *        end    the problem's episode ends when the tick reports first_bad >= 0 (end_reason 1, diverged) or first_fall >= 0 (end_reason 2, fell);
 *               with both, fell wins when first_fall <= first_bad.  end_step is that step as a global index.  The ending tick is logged and folded
 *               in full, and the problem's state is the ending tick's final state (hsddp_sim.h: a diverged sample keeps the state it had).
 *      From then on the problem is FROZEN: its state, row and log do not change, and its entry of the handle's initial condition is no longer
 *      written - not by the ending tick either, so its later solves go on from the state its last whole tick began from.  Its lane quad still runs
 *      in every later walk (from the frozen state) and its results are ignored.
 *   5. The pending impact: if the tick's last step is the last knot of its phase and that phase has a touchdown, the window the caller moves to no
 *      longer contains the reset map, and hsddp_sim_run returns the state in front of it.  k_episode_impact then applies the phase's reset map
 *      to the states of the problems that are still alive (the contact solve of the walk in mode 1 with the phase's touchdown set), and
 *      n_impacts counts the launch.  The log's last entry stays the state in front of the map, as in a simulation's trajectory.
 *   6. The hand-off: the states of the problems still alive are written into the handle's initial condition on the device.  The handle is
 *      otherwise left bit for bit as it was (its kernel table, hsddp_get_kernel_times, gains the device times of k_episode_commit and
 *      k_episode_impact).  tick += 1.  Everything is in place on return, on the handle's stream, as for hsddp_sim_run.
 *
 * Also HSDDP_EINVAL with nothing changed: n_exec <= 0 or max_ticks <= 0 or a window that does not hold n_exec leading whole-body knots at
 * hsddp_episode_create, a NULL argument, [b0, b0+nb) outside the batch, hsddp_episode_get_log on an object created without keep_log.  Y of a tick
 * whose walk kept no force records stays zero.  Destroy the object before its handle.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_EPISODE_H
#define HSDDP_EPISODE_H
#include "hsddp_sim.h"
#include "hsddp_mc.h"
#include "hsddp_grf.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_episode hsddp_episode_t;
typedef struct hsddp_episode_row {
    double dev_q, dev_v, min_height, max_torque;
    double min_fz, min_cone, max_fz;
    double track_cost;
    int n_sat, n_slip;
    int first_slip, steps;
    int bad_solves, end_reason;      /* end_reason: 0 alive, 1 diverged, 2 fell */
    int end_step, pad;               /* end_step: global step index, -1 while alive */
} hsddp_episode_row_t;               /* 96 bytes */

int hsddp_episode_create(hsddp_handle_t *h, int n_exec, int max_ticks, int keep_log, hsddp_episode_t **out);
void hsddp_episode_destroy(hsddp_episode_t *e);
int hsddp_episode_reset(hsddp_episode_t *e, const double *x0 /* [B][36] */, int src_device);
int hsddp_episode_advance(hsddp_episode_t *e, const hsddp_mc_dist_t *dist /* or NULL */, const double *kick /* [B][36] or NULL */, int kick_device);
/* rows [nb] and, unless NULL, the current states [nb][36] of problems [b0, b0+nb) (host destinations) */
int hsddp_episode_get_rows(hsddp_episode_t *e, int b0, int nb, hsddp_episode_row_t *rows, double *x_now);
/* the log of problems [b0, b0+nb): X [nb][max_ticks n_exec + 1][36], U and Y [nb][max_ticks n_exec][12] (host destinations, NULL skips one) */
int hsddp_episode_get_log(hsddp_episode_t *e, int b0, int nb, double *X, double *U, double *Y);
/* the current states on the device, [B][36]: valid until the object is destroyed, rewritten by every reset and advance */
const double *hsddp_episode_device_state(hsddp_episode_t *e);
/* the internal simulation object: for hsddp_grf_set only */
hsddp_sim_t *hsddp_episode_sim(hsddp_episode_t *e);
/* ticks advanced since the last reset, problems still alive, reset maps applied by hsddp_episode_advance since the last reset (NULL skips one) */
int hsddp_episode_status(hsddp_episode_t *e, int *tick, int *n_alive, int *n_impacts);

#ifdef __cplusplus
}
#endif
#endif
