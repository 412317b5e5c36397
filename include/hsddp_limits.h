/*
 * hsddp_limits.h — per-problem constraint limits for whole-body phases, on top of include/hsddp.h (libhsddp_hip.so).
 *
 * The limits of the path constraints of a phase live in its descriptor, one set for the whole batch: torque_limit, joint_lb / joint_ub, h_min, mu,
 * jointspeed_lb / jointspeed_ub.  This header gives every problem of the batch a row of its OWN limits, so that one batch can hold robots that plan
 * with different friction pyramids or actuator limits - a robot of an episode (include/hsddp_episode.h) that stands on ice can plan with the ice's
 * coefficient, a study of weak actuators can plan each robot with its own torque limit.
 *
 * A row is 12 doubles:   torque_limit | joint_lb[3] | joint_ub[3] | h_min | mu | jointspeed_lb | jointspeed_ub | pad
 * The values are ABSOLUTE (newton-metres, radians, metres, a friction coefficient), not scales.  An entry that is NaN means: this problem uses the
 * phase descriptor's value for this limit, in every phase.  For every WHOLE-BODY phase i of the current window and of every later one, problem b
 * uses its row's entry in place of the descriptor's field wherever the entry is set.  The value stands exactly where the descriptor's value stood,
 * in the same expression order: a batch-1 problem whose descriptor carries the value is the same arithmetic.
 *
 * NOT covered: ground_height (include/hsddp_touchdown.h owns it); the ReB and AL parameters (delta, eps, sigma, lambda), which are per problem as
 * they always were and start from the descriptor's reb_*; single-rigid-body and kinodynamic phases, which store the rows and do not use them.  A
 * limit whose constraint flag is off in a phase (c_torque = 0 and so on) is stored and unused there.
 *
 * hsddp_limits_set(h, b0, nb, rows, src_device)      rows: [nb][12]
 *   - The first call creates the table with every entry NaN, then writes [b0, b0+nb).  Later calls overwrite their range only.
 *   - src_device = 0: host memory, checked (every entry NaN or finite; torque_limit > 0, mu > 0; joint_lb[j] < joint_ub[j] and jointspeed_lb <
 *     jointspeed_ub where both are given; pad is ignored), reusable on return.  src_device = 1: device memory on the handle's device; the host does
 *     not read it.
 * hsddp_limits_get(h, phase, b0, nb, rows)           the values in use for that phase, host destination: the descriptor's where nothing is set, and
 *   for every problem when no table is set.
 * hsddp_limits_clear(h)
 *   - Afterwards exactly the kernels of before are launched; a solve is bit-identical to one on a handle that never had limits.
 * hsddp_episode_plan_friction(e, kappa)              mu of robot b <- kappa * mu_s[mu_of[b]], 0 < kappa <= 1
 *   - Reads the friction table the episode simulates with (include/hsddp_friction.h) on the device, in one launch; nothing is uploaded.  The other
 *     entries of the rows are untouched; a handle without a table gets one with every other entry NaN.  The product is one fp64 multiply.
 *   - HSDDP_EINVAL when the episode has no friction set or kappa is out of range.
 * While a table is set and the window has a whole-body phase, hsddp_solve and the step API (hsddp_hybrid_rollout, hsddp_LQ_approximation, the
 *   line-search probes) launch the kernels that read it (k_rollout_lim, k_rollout_quad_lim, k_lq_lim; hsddp_get_kernel_times lists their launches
 *   as k_rollout_lim, k_lq_lim and k_ls_probe_lim).  Terminal knots read no path-constraint limit and run what they ran.  Limits, the cost-weight
 *   scales of include/hsddp_weights.h and the touchdown heights of include/hsddp_touchdown.h combine freely.
 * The table belongs to the HANDLE, not to a phase: it survives hsddp_reconfigure, which resolves the rows against the new window's descriptors in one
 *   small launch (k_pack_limits: the only added work per tick).  hsddp_warm_start_phase does not copy it; every candidate handle of an ensemble has
 *   its own.
 * Allocation: one block (and, for the combination with touchdown heights, that header's table), made by the first call and freed by hsddp_destroy;
 *   a warm tick allocates nothing (hsddp_debug_malloc_count).
 * HSDDP_EINVAL, with nothing changed: a NULL handle or source, a range outside the batch, nb <= 0, a phase outside the window, a bad host value.
 * HSDDP_ENOTSUP: an fp32 handle.
 *
 * Out of scope: limits on single-rigid-body / kinodynamic phases; fp32 handles; limits that vary by knot or by leg; per-problem ReB / AL initial
 * parameters; a torque limit derived from the plant gains of include/hsddp_plant.h.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_LIMITS_H
#define HSDDP_LIMITS_H
#include "hsddp.h"
#include "hsddp_episode.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HSDDP_LIMITS_ROW 12      /* torque_limit | joint_lb[3] | joint_ub[3] | h_min | mu | jointspeed_lb | jointspeed_ub | pad */

int hsddp_limits_set(hsddp_handle_t *h, int b0, int nb, const double *rows, int src_device);
int hsddp_limits_get(hsddp_handle_t *h, int phase, int b0, int nb, double *rows);
int hsddp_limits_clear(hsddp_handle_t *h);
int hsddp_episode_plan_friction(hsddp_episode_t *e, double kappa);

#ifdef __cplusplus
}
#endif
#endif
