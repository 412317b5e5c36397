/*
 * hsddp_terrain.h — terrain height maps and early swing-foot touchdown in a closed-loop simulation object (include/hsddp_sim.h, include/hsddp_mc.h,
 * include/hsddp_grf.h, include/hsddp_substep.h, include/hsddp_contact.h, include/hsddp_episode.h; libhsddp_hip.so).
 *
 * With hsddp_contact.h alone the ground is one plane, and only SCHEDULED stance feet are tested against it: a swing foot that reaches the ground before
 * the schedule attaches it passes through.  This header gives the ground a height per place and per sample, and lets a swing foot land when it
 * arrives.  Both extend the rules of hsddp_contact.h and are DORMANT while that rule is off.
 *
 * Terrain.  A piecewise-constant height grid H [n_maps][ny][nx] of doubles with origin (x0, y0) and cell size (cx, cy).  For a foot point p
 *     ix = clamp(floor((p_x - x0) / cx), 0, nx - 1),  iy = clamp(floor((p_y - y0) / cy), 0, ny - 1),  z_g(p) = z_ground + H[m][iy][ix]
 * with z_ground of hsddp_contact_set and m = map_of[b][r], an int [batch][n_samples] table given with the grid (NULL: map 0 for every sample) - so every
 * sample of a Monte-Carlo run can have a terrain of its own.  Outside the grid the edge cell holds (a NaN coordinate reads cell 0).  The contact normal
 * stays vertical, an attached foot stays where it was attached, and a foot that moves sideways into a riser is not stopped.
 *
 * Early touchdown (early != 0, threshold w_td >= 0).  A sample's state becomes (x, F, E): F as in hsddp_contact.h, E the set of SWING feet (not in the
 * phase's stance set C) that are currently attached.  Per substep of a live sample, extending the four rules of hsddp_contact.h:
 *   1. Landing.  Tested feet: (F n C) u (early ? (not C) \ E : nothing).  T = { f tested : p_z <= z_g(p) and w_z < thr_f }, thr = 0 for a scheduled
 *      stance foot (as before) and thr = -w_td for a swing foot: a foot that has just lifted off on schedule sits at the ground with w_z = +-1e-17, and
 *      without the threshold rounding would decide its test.  The impact on T alone is unchanged.  Then F <- F \ T, n_land += |T n C|, and
 *      E <- E u (T \ C), n_early += |T \ C|, first_early is set to the control step if it is unset.  max_lift takes p_z - z_g(p) over F n C as before;
 *      max_pen takes z_g(p) - p_z over T.
 *   2. Lift-off.  The attached set of every solve is A = (C \ F) u E.  The foot with the smallest lambda_z below fz_rel leaves A, lowest leg on a tie:
 *      a stance foot goes into F (n_release, first_release as before), a foot of E simply leaves E (n_early_release).  At most four repeats.
 *   3. Step and divergence test.  Unchanged.
 *   4. Phase change.  F <- F n C_new and E <- E \ C_new: such a foot is now an ordinary attached stance foot.  Scheduled touchdowns and the pending
 *      impact of an episode stay on schedule; they now act on a foot that is already at rest.
 *
 * Force records run over the attached feet of a substep's last solve, so feet of E count as stance feet there.
 *
 * Runs and episodes.  hsddp_sim_run and hsddp_mc_run start every sample with E empty.  An episode keeps E per robot by leg beside F under the same
 * rules: it survives hsddp_reconfigure, is cleared by hsddp_episode_reset, and a frozen robot keeps the E it froze with.
 *
 * The record of a sample, hsddp_terrain_row_t:
 *   first_early      control step of the first early touchdown, -1 if none      n_early      early touchdowns
 *   n_early_release  releases of feet of E                                       n_held       (foot, substep) pairs of E at a substep's last solve,
 *   early_final      bit l = leg l is in E at the end of the run                              for samples alive when the substep began
 *   max_pen          largest z_g(p) - p_z over the landing sets T, 0 if no foot ever landed
 *
 * Rules:
 *   - HSDDP_EINVAL with nothing changed: a NULL sim; and for on != 0 a NULL t or H, a non-finite x0, y0, cx, cy, w_td or height, cx or cy <= 0,
 *     w_td < 0, a size outside 1 <= nx, ny <= 1024, 1 <= n_maps <= 4096, n_maps nx ny <= 2^22, a map_of entry outside [0, n_maps).
 *     HSDDP_ENOTSUP: on != 0 for an fp32 handle.  on = 0 ignores t, H and map_of.
 *   - H and map_of are host pointers; the call copies them.
 *   - Dormancy: with the contact rule off, or the terrain off, exactly the kernels of the headers above are launched and a run is bit-identical to one
 *     before this header existed.  The call may be made while the contact rule is off; the terrain acts from the first run with both on.
 *   - A set call may allocate (the first one, and when the grid grows); runs never allocate (hsddp_debug_malloc_count).  The handle is left bit for
 *     bit as it was.
 *   - hsddp_terrain_get_params reads back what later runs use (on = 0 and zeros on a fresh object).
 *   - hsddp_terrain_get returns the rows of the LAST run; HSDDP_EINVAL if that run had the terrain dormant, for a bad range or a NULL argument.
 *   - hsddp_episode_sim(e) is accepted, as by hsddp_contact_set.  Its rows are those of the last tick.
 *
 * Out of scope: sloped contact normals and risers that stop a foot sideways; sliding friction; the sign of landing impulses; fp32 handles; grids that
 * already live in device memory.  Terrain-aware planning is include/hsddp_touchdown.h: it gives the solver the grid's height at each reference foothold
 * as the touchdown height of that problem and leg (hsddp_episode_plan_terrain for an episode's own terrain).
 */
#ifndef HSDDP_TERRAIN_H
#define HSDDP_TERRAIN_H
#include "hsddp_contact.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int nx, ny, n_maps, early;
    double x0, y0, cx, cy, w_td;
} hsddp_terrain_t;

typedef struct {
    int first_early, n_early, n_early_release, n_held, early_final, pad;
    double max_pen;
} hsddp_terrain_row_t;

int hsddp_terrain_set(hsddp_sim_t *s, int on, const hsddp_terrain_t *t, const double *H, const int *map_of);
int hsddp_terrain_get_params(hsddp_sim_t *s, int *on, hsddp_terrain_t *t);
int hsddp_terrain_get(hsddp_sim_t *s, int b0, int nb, hsddp_terrain_row_t *rows);      /* rows [nb][n_samples] of the last run */

#ifdef __cplusplus
}
#endif
#endif
