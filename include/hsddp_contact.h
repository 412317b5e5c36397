/*
 * hsddp_contact.h — unilateral ground contact in a closed-loop simulation object (include/hsddp_sim.h, include/hsddp_mc.h, include/hsddp_grf.h,
 * include/hsddp_substep.h, include/hsddp_episode.h; libhsddp_hip.so).
 *
 * A simulation glues every scheduled stance foot to the ground as a BILATERAL constraint: the ground gives whatever force the constraint asks
 * for, a pull included (hsddp_grf.h only counts such steps).  With the rule of this header switched on the ground can only push: a stance foot
 * whose normal force falls below fz_rel is released, moves freely, and is attached again when it comes back down to the ground.
 *
 * A sample's state becomes (x, F): F is the set of scheduled stance feet that are currently FREE.  hsddp_contact_set(sim, on, fz_rel, z_ground)
 * switches the rule on for every later run of the object.  The ground is flat at world height z_ground, which is compared with the foot point
 * the touchdown constraint uses (the point whose velocity the contact constraint holds at zero).
 *
 * Let C be the stance set of the step's phase and S >= 1 the substeps of hsddp_substep.h.  Everything hsddp_substep.h does once per control step
 * is unchanged.  In each substep a live sample does:
 *   1. Landing.  p, w: position and velocity of the feet at the substep's start state.  T = { f in F n C : p_z[f] <= z_ground and w_z[f] < 0 }.
 *      If T is not empty: the impact map on the feet of T only - lambda = G^-1 (-J_T v), Gram damping 0, x <- (q, v+), what the reset map of a
 *      scheduled touchdown does - then F <- F \ T and n_land += |T|.  max_lift takes p_z - z_ground of every foot of F n C here.
 *   2. Lift-off.  A = C \ F; the contact solve of hsddp_substep.h (the phase's bg_alpha, Gram damping 1e-12) on A.  While A is not empty and
 *      min over A of lambda_z < fz_rel: the foot with the smallest lambda_z, lowest leg index on a tie, moves from A into F; n_release += 1;
 *      first_release is set to the control step if it is unset; solve again.  At most four repeats.  An empty A is free flight.
 *   3. Step.  The Euler step of dt / S with the accelerations of the LAST solve; the divergence test as in hsddp_substep.h.  A sample that fails
 *      keeps the state the failing step was taken from (behind a landing of that substep, if there was one) and the F and counters of that
 *      moment; nothing further is counted.
 *   4. Phase boundaries.  F <- F n C_new at a phase change.  Scheduled touchdowns - the reset map behind the last substep of a phase's last
 *      knot, and the pending impact of an episode - are unchanged and happen on schedule.  Consequence: a foot the schedule attaches in mid-air
 *      is a stance foot with F not holding it; its constraint pulls, it is released in its next substep, and it lands at z_ground like any other.
 *
 * Runs and episodes.  hsddp_sim_run and hsddp_mc_run start every sample with F empty.  An episode keeps F per robot in device memory from tick to
 * tick; it is indexed by leg, so it survives hsddp_reconfigure; hsddp_episode_reset clears it; a frozen robot keeps the F it froze with.
 *
 * Force records (hsddp_grf_set on) run over the ATTACHED feet of the last solve of each substep.  A free foot's force is exactly 0 and it is no
 * stance foot for min_fz, min_cone, max_fz and n_slip.  Y[b][r][s] is the last solve of substep 0.  Hence min_fz >= fz_rel whenever it is finite.
 * With the rule on the records are always computed; if hsddp_grf_set never switched them on they go to an internal block and hsddp_grf_get
 * keeps answering HSDDP_EINVAL.
 *
 * The record of a sample, hsddp_contact_row_t:
 *   first_release  control step of the first release, -1 if none        n_release  feet released
 *   n_land         feet landed                                           n_free     (foot, substep) pairs of F n C at the last solve of a
 *   free_final     bit l = leg l is in F at the end of the run                      substep, for samples alive when the substep began
 *   max_lift       largest p_z - z_ground of a landing test (step 1), 0 if no foot was ever tested
 *
 * Rules:
 *   - HSDDP_EINVAL with nothing changed: a NULL argument, a non-finite fz_rel or z_ground.  HSDDP_ENOTSUP: on != 0 for an fp32 handle.
 *   - on = 0, or an object on which the call was never made, launches exactly the kernels of hsddp_sim.h, hsddp_mc.h, hsddp_grf.h and
 *     hsddp_substep.h: a run is bit-identical to one before this header existed.  The thresholds of an on = 0 call are not kept.
 *   - The first on != 0 call allocates; later calls and all runs allocate nothing (hsddp_debug_malloc_count).  The handle is left bit for bit as
 *     it was, as by every simulation call.
 *   - hsddp_contact_get_params reads back what later runs use (on = 0, thresholds 0 on a fresh object).
 *   - hsddp_contact_get returns the rows of the LAST run; HSDDP_EINVAL if that run had the rule off, for a bad range or a NULL argument.
 *   - hsddp_episode_sim(e) is accepted, as for hsddp_grf_set and hsddp_substep_set.  Its rows are those of the last tick.
 *
 * Out of scope: sliding friction (cone violations are still only counted, the foot does not slide); negative impulses in impacts (the impact map is
 * the bilateral one on T, whatever sign its impulse has); fp32 handles and windows that do not lead with whole-body knots.  Early touchdown of a SWING
 * foot (here only scheduled stance feet are tested against the ground) and terrain (here the ground is one plane) are include/hsddp_terrain.h, which
 * extends the rules above.
 */
#ifndef HSDDP_CONTACT_H
#define HSDDP_CONTACT_H
#include "hsddp_sim.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int first_release, n_release, n_land, n_free, free_final, pad;
    double max_lift;
} hsddp_contact_row_t;

int hsddp_contact_set(hsddp_sim_t *s, int on, double fz_rel, double z_ground);
int hsddp_contact_get_params(hsddp_sim_t *s, int *on, double *fz_rel, double *z_ground);
int hsddp_contact_get(hsddp_sim_t *s, int b0, int nb, hsddp_contact_row_t *rows);      /* rows [nb][n_samples] of the last run */

#ifdef __cplusplus
}
#endif
#endif
