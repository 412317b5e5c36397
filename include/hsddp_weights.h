/*
 * hsddp_weights.h — per-problem cost-weight scales for whole-body phases, on top of include/hsddp.h (libhsddp_hip.so).
 *
 * The tracking weights q, r and qf of a phase live in its descriptor, one set for the whole batch.  This header gives every problem of the batch a
 * row of SCALES on top of them, so that one batch can hold robots that plan with different weightings - the controller-tuning use of the closed-loop
 * episodes (include/hsddp_episode.h).
 *
 * A row is 84 doubles: sq[36] | sr[12] | sqf[36].  For every WHOLE-BODY phase i of the current window and of every later one, problem b uses
 *   running cost    q_i[j] * sq_b[j]  and  r_i[j] * sr_b[j]  (j < 12)   in place of q_i[j] and r_i[j],
 *   terminal cost   qf_i[j] * sqf_b[j]                                  in place of qf_i[j].
 * The product is formed once per weight and stands exactly where the descriptor's weight stands, in the same expression order: a batch-1 problem
 * whose descriptor carries the product q * sq is the same arithmetic.
 *
 * NOT scaled: the foot costs (w_foot_reg, w_swing_pos, w_swing_vel) and w_td_vel; every constraint and its ReB / AL parameters; single-rigid-body and
 * kinodynamic phases; the exports and the ensembles' winner selection; and the episode commit's track_cost (hsddp_episode.h), which goes on using the
 * DESCRIPTOR's weights on purpose: it is the common yardstick across robots that plan with different weights.
 *
 * hsddp_weights_set(h, b0, nb, scales, src_device)      scales: [nb][84]
 *   - The first call creates the table with every problem at 1.0, then writes [b0, b0+nb).  Later calls overwrite their range only.
 *   - src_device = 0: host memory, checked (finite; sq, sqf >= 0; sr > 0), reusable on return.  src_device = 1: device memory on the handle's device;
 *     the host does not read it.
 * hsddp_weights_get(h, b0, nb, scales)                  the rows in use, host destination: 1.0 everywhere when none are set
 * hsddp_weights_clear(h)
 *   - Afterwards exactly the kernels of include/hsddp.h are launched; a solve is bit-identical to one on a handle that never had scales.
 * While a table is set, hsddp_solve and the step API (hsddp_hybrid_rollout, hsddp_LQ_approximation, the line-search probes) launch the kernels that
 *   read it (k_rollout_pw, k_rollout_quad_pw, k_rollout_quad_term_pw, k_lq_pw; hsddp_get_kernel_times lists their launches as k_rollout_pw, k_lq_pw
 *   and k_ls_probe_pw).  A window without a whole-body phase stores the scales and does not use them.  Scales and the touchdown heights of
 *   include/hsddp_touchdown.h combine freely.
 * The table belongs to the HANDLE, not to a phase: it survives hsddp_reconfigure (unlike references and touchdown heights), so an episode sets it once.
 *   hsddp_warm_start_phase does not copy it; every candidate handle of an ensemble has its own.
 * Allocation: one table (and, for the combination with touchdown heights, that header's table), made by the first call and freed by hsddp_destroy;
 *   a warm tick allocates nothing (hsddp_debug_malloc_count).
 * HSDDP_EINVAL, with nothing changed: a NULL handle or source, a range outside the batch, nb <= 0, a bad host value.  HSDDP_ENOTSUP: an fp32 handle.
 *
 * Out of scope: scales on single-rigid-body / kinodynamic phases, on the foot costs or on constraint parameters (per-problem constraint LIMITS are
 * include/hsddp_limits.h); fp32 handles; weights that vary by knot; a tuner.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_WEIGHTS_H
#define HSDDP_WEIGHTS_H
#include "hsddp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HSDDP_WEIGHTS_ROW 84      /* sq[36] | sr[12] | sqf[36] */

int hsddp_weights_set(hsddp_handle_t *h, int b0, int nb, const double *scales, int src_device);
int hsddp_weights_get(hsddp_handle_t *h, int b0, int nb, double *scales);
int hsddp_weights_clear(hsddp_handle_t *h);

#ifdef __cplusplus
}
#endif
#endif
