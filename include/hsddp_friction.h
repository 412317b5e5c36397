/*
 * hsddp_friction.h — Coulomb friction in a closed-loop simulation object: stance feet that slide (include/hsddp_sim.h, include/hsddp_mc.h,
 * include/hsddp_grf.h, include/hsddp_substep.h, include/hsddp_contact.h, include/hsddp_terrain.h, include/hsddp_episode.h; libhsddp_hip.so).
 *
 * With the headers above an attached foot is held by a three-axis bilateral constraint: the ground supplies any horizontal force the constraint asks
 * for, and hsddp_grf.h only counts the steps on which that force leaves the friction pyramid.  This header lets such a foot slide.  It extends the
 * rules of hsddp_contact.h (and of hsddp_terrain.h when the terrain is on) and is DORMANT while the contact rule is off.  The ground normal is world z.
 *
 * The table.  mu [n_mu][2] of doubles, a row = (mu_s, mu_k) with 0 <= mu_k <= mu_s, and mu_of [batch][n_samples], the row of a sample (NULL: row 0 for
 * every sample) - the shape of hsddp_plant_set and hsddp_terrain_set.  v_stick >= 0 is the speed below which a sliding foot sticks again.
 *
 * State.  A sample's state becomes (x, F, E, Sl, n): F and E as in the headers above, A = (C \ F) u E the attached feet of a solve; Sl, a subset of A,
 * the SLIDING feet; n_f >= 0 the lagged normal force of a sliding foot; and, inside a substep only, t^_f, a unit vector in the world x-y plane, and the
 * flag FRESH (f joined Sl in this substep).
 *
 * Solve.  Every mode-0 solve of a substep (forwardDynamics; the impacts of mode 1 are unchanged, and a foot attached by an impact is sticking) treats
 * an attached foot in one of two ways.
 *   sticking  the three-row constraint of hsddp_contact.h.
 *   sliding   only the z row is constrained, with the same Baumgarte term and the same 1e-12 damping on that row; lambda_x = lambda_y = 0.  A known
 *             tangential force f_t acts on the foot point and enters the generalised force as J_f^T f_t:
 *               fresh:      f_t = mu_k n_f t^_f.  Friction opposes the impending motion: t^_f = lambda_t / |lambda_t| of the stick solve that put the
 *                           foot into Sl (t^_f = 0 if that lambda_t is exactly 0).
 *               otherwise:  with w_t the tangential velocity of the foot point at the solve's own state, f_t = -mu_k n_f w_t / |w_t| if |w_t| > v_stick;
 *                           else the foot RE-STICKS: it leaves Sl, this solve holds it with all three rows, and n_restick += 1.
 * Per substep of a live sample, extending the rules of hsddp_contact.h and hsddp_terrain.h:
 *   1. Landing.  Unchanged.  The first solve of a substep decides nothing about friction if a landing impact follows it: its re-sticks are taken by
 *      the solve behind the impact, at the velocities the impact left.
 *   2. Lift-off.  Unchanged; a foot that is released leaves Sl.  Release comes first: the onset test below runs only behind a solve that released
 *      nothing.
 *   2b. Onset.  Among the STICKING attached feet of that solve take m_f = mu_s lambda_z - sqrt(lambda_x^2 + lambda_y^2), the circular cone, which
 *      lies inside the pyramid of hsddp_grf.h at equal mu.  If the smallest m_f is negative, that foot (lowest leg on a tie) joins Sl with
 *      n_f = max(lambda_z, 0) of this solve and t^_f as above, fresh; n_onset += 1, first_slide is set to the control step if it is unset, and the solve
 *      is repeated.  Within a substep a foot moves one way - slide -> stick (a re-stick), stick -> slide (fresh), attached -> free - so the repeats end.
 *   3. End of a substep, at the solve whose accelerations are integrated: every attached sliding foot takes n_f <- max(lambda_z, 0) of that solve, every
 *      fresh flag clears, n_slide += |Sl n A|, and over those feet distance += |w_t| dt / S and max_speed = max(max_speed, |w_t|) with the velocity
 *      that solve saw.  Then the step and the divergence test, unchanged: a sample that fails it keeps its state, Sl, n and counters of that moment.
 *   4. Phase change.  Sl <- Sl n A with the new stance set: a foot that leaves the stance set leaves Sl, a foot of E that becomes a scheduled stance
 *      foot stays what it was.
 * Nothing a solve reads changes between repeats of a solve with the same sets, so a repeat returns the same numbers.
 *
 * Force records (hsddp_grf.h).  Y, min_fz and max_fz run over all attached feet; for a sliding foot Y holds (f_t.x, f_t.y, lambda_z).  min_cone,
 * first_slip and n_slip run over the STICKING attached feet only.  With hsddp_grf_set(mu = mu_s) therefore min_cone >= 0 on every sample, up to the
 * rounding of the solve.
 *
 * Runs and episodes.  hsddp_sim_run and hsddp_mc_run start every sample with Sl empty.  An episode keeps (Sl, n_f) per robot and leg beside F and E
 * under the same rules: they survive hsddp_reconfigure, are cleared by hsddp_episode_reset, and a frozen robot keeps its own.
 *
 * The record of a sample, hsddp_friction_row_t:
 *   first_slide  control step of the first onset, -1 if none          n_onset    onsets
 *   n_slide      (foot, substep) pairs of Sl at a substep's last      n_restick  re-sticks
 *                solve, for samples alive when the substep began      slide_final  bit l = leg l is in Sl at the end of the run
 *   max_speed    largest |w_t| of a sliding foot at such a solve      distance   sum of |w_t| dt / S over those pairs, all four feet
 *
 * Rules:
 *   - HSDDP_EINVAL with nothing changed: a NULL sim; and for on != 0 a NULL params or mu, n_mu < 1 (or above 65536), a non-finite or negative v_stick,
 *     mu_s or mu_k, mu_k > mu_s, a mu_of entry outside [0, n_mu).  HSDDP_ENOTSUP: on != 0 for an fp32 handle.  on = 0 ignores the other arguments.
 *   - mu and mu_of are host pointers; the call copies them.
 *   - Dormancy: with the contact rule off, or friction off, exactly the kernels of the headers above are launched and a run is bit-identical to one
 *     before this header existed.  With the terrain off the friction walk runs on an internal flat one-cell map without early touchdown, which is the
 *     contact rule alone; hsddp_terrain_get then refuses as it does for a run with the terrain dormant.
 *   - A run with friction AND the per-sample plant of hsddp_plant.h both acting answers HSDDP_ENOTSUP; it is never silently ignored.  (Both calls may be
 *     made; the refusal is the run's.)  hsddp_sim_run, hsddp_mc_run and hsddp_episode_advance ask first: nothing is allocated, copied or launched, an
 *     episode's tick count, window binding and latency stash stay what they were.
 *   - The first on call allocates (and a later one whose table is larger than every earlier one); other calls and all runs allocate nothing
 *     (hsddp_debug_malloc_count).  The handle is left bit for bit as it was.
 *   - hsddp_friction_get_params reads back what later runs use (on = 0 and zeros on a fresh object).
 *   - hsddp_friction_get returns the rows of the LAST run; HSDDP_EINVAL if that run had friction dormant, for a bad range or a NULL argument.
 *   - hsddp_episode_sim(e) is accepted, as by hsddp_contact_set.  Its rows are those of the last tick.
 *
 * Pulling feet.  hsddp_contact.h keeps a foot attached while lambda_z >= fz_rel, and fz_rel may be negative.  A foot with fz_rel <= lambda_z < 0 is outside
 * the cone at ANY mu_s: it joins Sl with n_f = 0 and slides freely until it pushes again.  With fz_rel = 0 such a foot is released before the onset test.
 *
 * Limits.  The friction is explicit in the normal force: n_f is that of the previous substep, a first-order error in dt / S, as the plant's viscous
 * term is in the velocity.  A fast reversal can step over v_stick and chatter for a few substeps; sub-stepping is the remedy.  Out of scope: friction
 * per terrain cell; tangential impulses in impacts; anisotropic friction; an implicit (non-symmetric) solve; fp32 handles; the combination with
 * hsddp_plant_set (refused, see above).
 */
#ifndef HSDDP_FRICTION_H
#define HSDDP_FRICTION_H
#include "hsddp_terrain.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double v_stick;
    int n_mu, pad;
} hsddp_friction_t;

typedef struct {
    int first_slide, n_onset, n_slide, n_restick, slide_final, pad;
    double max_speed, distance;
} hsddp_friction_row_t;

int hsddp_friction_set(hsddp_sim_t *s, int on, const hsddp_friction_t *params, const double *mu, const int *mu_of);
int hsddp_friction_get_params(hsddp_sim_t *s, int *on, hsddp_friction_t *params);
int hsddp_friction_get(hsddp_sim_t *s, int b0, int nb, hsddp_friction_row_t *rows);      /* rows [nb][n_samples] of the last run */

#ifdef __cplusplus
}
#endif
#endif
