/*
 * hsddp_sim.h — batched closed-loop rollouts of a solved whole-body policy from perturbed initial states, on top of include/hsddp.h
 * (libhsddp_hip.so).
 *
 * A solve leaves a feedback policy on the device for every problem of the batch: Xbar, Ubar, K.  A simulation object applies that policy to
 * R initial states per problem over the first n_steps control knots of the handle, walking the whole-body phases in order as
 * hsddp_export_mpc_command does.  For problem b, sample r:
 *
 *     x = x0[b][r]
 *     per control knot (phase i, k):   u = Ubar_{i,k} + K_{i,k} (x - Xbar_{i,k})
 *                                      x = whole-body contact dynamics of phase i, forward Euler (WBM.cpp:17-57, 368-424)
 *     at the end of phase i, if the window goes on:   x = reset map of the phase (the impact on the feet that touch down,
 *                                      WBM.cpp:178-206, 427-456; the identity if none does)
 *
 * which is what hsddp_hybrid_rollout(eps = 0, MS = 0) computes from the initial condition x0[b][r] - without costs, defects and constraint
 * values, and without a write to the handle: its trajectories and its contact-solve cache are as they were.  The controller side of the
 * reference does the same one state at a time (MHPC/MHPC-Trajopt/test/testTrajOptInLoop.cpp).
 *
 * Per (b, r) a row comes back:
 *     dev_q, dev_v   largest |x - Xbar| over the positions (0..17) / the velocities (18..35), taken at every state a control is applied from
 *                    and at the final state (against the knot behind the last step)
 *     min_height     smallest x[2] over the same states
 *     max_torque     largest |u|
 *     first_bad      first step whose new state fails the rollout's divergence test (squared norm above 1e12, or NaN), else -1.  Such a sample
 *                    keeps the state it had before that step and records nothing further; the other samples are unaffected.
 * and the final state x_final (before any reset map behind the last step).  With keep_traj the states [B][R][n_steps+1][36] and controls
 * [B][R][n_steps][12] are kept too: entry j < n_steps is the state u_j is applied from (behind a reset map, where one precedes it), entry
 * n_steps the final state.
 *
 * Rules:
 *   - fp64 whole-body knots only.  A window that reaches a phase that is not whole-body (the SRB tail) is HSDDP_EINVAL, as for the command
 *     export; it may end exactly at the last whole-body knot.  An fp32 handle has no whole-body phase and is refused by the same rule.
 *   - hsddp_sim_create allocates everything; hsddp_sim_run allocates nothing (hsddp_debug_malloc_count is unchanged by it).
 *   - hsddp_sim_run uses the handle's CURRENT policy and runs on the handle's stream: a call on the handle like any other, which the caller
 *     serialises with hsddp_solve.  x0 is [B][R][36]: host memory (src_device = 0, reusable on return) or device memory on the handle's
 *     device (src_device = 1, for example a torch tensor, read in place).  The results are in place on return.
 *   - hsddp_reconfigure makes the object stale: hsddp_sim_run returns HSDDP_EINVAL until a new object is created.
 *   - Per-problem references (hsddp_refs.h) play no part: the simulation reads no reference.
 *   - HSDDP_EINVAL with nothing changed: n_samples <= 0, n_steps <= 0, a NULL argument, [b0, b0+nb) outside the batch, hsddp_sim_get_traj on an
 *     object created without keep_traj.
 *   - Destroy the object before its handle.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_SIM_H
#define HSDDP_SIM_H
#include "hsddp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_sim hsddp_sim_t;
typedef struct hsddp_sim_row {
    double dev_q, dev_v, min_height, max_torque;
    int first_bad, pad;
} hsddp_sim_row_t;

int hsddp_sim_create(hsddp_handle_t *h, int n_samples, int n_steps, int keep_traj, hsddp_sim_t **out);
int hsddp_sim_run(hsddp_sim_t *s, const double *x0 /* [B][R][36] */, int src_device);
/* rows [nb][R] and, unless NULL, final states [nb][R][36] of problems [b0, b0+nb) of the last run (host destinations) */
int hsddp_sim_get_rows(hsddp_sim_t *s, int b0, int nb, hsddp_sim_row_t *rows, double *x_final);
/* states [nb][R][n_steps+1][36] and controls [nb][R][n_steps][12] of the last run (host destinations, NULL skips one) */
int hsddp_sim_get_traj(hsddp_sim_t *s, int b0, int nb, double *X, double *U);
/* final states of the last run on the device, [B][R][36]: valid until the object is destroyed, rewritten by every run */
const double *hsddp_sim_device_final(hsddp_sim_t *s);
int hsddp_sim_get_kernel_time_ms(hsddp_sim_t *s, float *ms);   /* device time of the kernel of the last run (HIP events) */
void hsddp_sim_destroy(hsddp_sim_t *s);

#ifdef __cplusplus
}
#endif
#endif
