/*
 * hsddp_touchdown.h — per-problem, per-foot touchdown heights and terrain-aware planning, on top of include/hsddp.h (libhsddp_hip.so).
 *
 * The touchdown constraint of a whole-body phase is the height of the feet that land at its end above the ground, h = foot_z - ground_height, with
 * ONE ground_height in the phase descriptor for the whole batch and all four feet.  This header lets the height differ per problem and per leg, fills
 * it from a terrain height grid (include/hsddp_terrain.h) at the reference footholds, and gives the MPC episodes (include/hsddp_episode.h) a call that
 * does so every tick from the terrain the episode already simulates on: the planner then lands where the simulated ground is.
 *
 * Heights are [nb][4] doubles, problem-major, by leg FL FR HL HR.
 *
 * hsddp_touchdown_set(h, phase, b0, nb, heights, src_device)
 *   - For a touchdown leg l of problem b of the phase, h = foot_z - heights[b][l] replaces foot_z - ground_height.  Entries of legs that do not touch
 *     down at the end of the phase are stored and returned but never read by a kernel.  The cost, the AL terms, max |h|, the stored constraint value,
 *     the LQ terminal knot and the AL update are unchanged: they read the stored value.
 *   - The first call on a phase switches it to per-problem heights: all problems start from the descriptor's ground_height, then [b0, b0+nb) take the
 *     given rows.  Later calls overwrite their range only.
 *   - src_device = 1: device memory on the handle's device.  src_device = 0: host memory, checked for finite values, reusable on return.
 * hsddp_touchdown_get(h, phase, b0, nb, heights, values)
 *   - heights: the heights in use (the shared value when the phase has none of its own).  values: by leg, the constraint values the last WRITING
 *     rollout stored, NaN for legs without a touchdown.  Host destinations; NULL skips.
 * hsddp_touchdown_clear(h, phase)       phase = -1: every phase
 *   - Returns the phase to the shared value.  With no phase left, exactly the kernels of include/hsddp.h are launched and a solve is bit-identical
 *     to one on a handle that never had heights.
 * Other calls: hsddp_reconfigure returns every phase of the new window to the shared value, as it does for references - a fleet sets its heights again
 *   after each reconfigure; hsddp_set_references on a phase keeps that phase's heights; hsddp_warm_start_phase, the ensembles and the exports are
 *   unaffected.
 * Allocation: one table owned by the handle, made by the first call and freed by hsddp_destroy; a tick of reconfigure -> set allocates nothing once
 *   warm (hsddp_debug_malloc_count).
 * HSDDP_EINVAL, with nothing changed: a NULL handle, a phase or range outside the window / batch, nb <= 0, NULL heights, a non-finite host value, a
 *   phase with no touchdown constraint.  HSDDP_ENOTSUP: a phase that is not whole-body (kinodynamic and single-rigid-body phases keep the shared
 *   value), an fp32 handle.
 *
 * hsddp_touchdown_from_terrain(h, t, H, map_of, z_ground, src_device)
 *   - Acts on every whole-body phase with a touchdown constraint, every problem and all four legs: height = z_ground + H[m][iy][ix], the cell that of
 *     the phase's TERMINAL reference foothold foot_pos[row h][3l .. 3l+1] - the problem's own row if the phase has per-problem references
 *     (include/hsddp_refs.h), the shared row otherwise - and m = map_of[b] (int [batch]; NULL: map 0).  The lookup is that of hsddp_terrain.h: clamped
 *     cell indices, edge cells hold outside the grid, a NaN coordinate reads cell 0.  One kernel launch for the whole window.
 *   - H [n_maps][ny][nx] and map_of are both host memory (src_device = 0, copied) or both device memory (1).  Validation as hsddp_terrain_set with
 *     on != 0 (t->early and t->w_td are not read); the VALUES of a device grid or map are not read by the host - a map index outside [0, n_maps) is
 *     clamped by the kernel.  A host grid is staged in a buffer of the handle that only grows.
 * hsddp_episode_plan_terrain(e)
 *   - The same launch, fed from the grid, z_ground and map_of[b][0] the episode's simulation object already holds on the device (hsddp_terrain_set,
 *     hsddp_contact_set on hsddp_episode_sim(e)); nothing is uploaded.  HSDDP_EINVAL if the episode has no terrain set.  To be called after
 *     hsddp_reconfigure (and after any hsddp_set_references) and before the solve.
 *
 * Out of scope: lifting the tracking references onto the terrain (hsddp_set_references does that), sloped contact normals, kinodynamic and
 * single-rigid-body phases, fp32 handles, adapting the schedule to an early touchdown.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_TOUCHDOWN_H
#define HSDDP_TOUCHDOWN_H
#include "hsddp.h"
#include "hsddp_terrain.h"
#include "hsddp_episode.h"
#ifdef __cplusplus
extern "C" {
#endif

int hsddp_touchdown_set(hsddp_handle_t *h, int phase, int b0, int nb, const double *heights, int src_device);
int hsddp_touchdown_get(hsddp_handle_t *h, int phase, int b0, int nb, double *heights, double *values);
int hsddp_touchdown_clear(hsddp_handle_t *h, int phase);
int hsddp_touchdown_from_terrain(hsddp_handle_t *h, const hsddp_terrain_t *t, const double *H, const int *map_of, double z_ground, int src_device);
int hsddp_episode_plan_terrain(hsddp_episode_t *e);

#ifdef __cplusplus
}
#endif
#endif
