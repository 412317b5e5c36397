/*
 * hsddp_refs.h — per-problem tracking references on top of include/hsddp.h (libhsddp_hip.so).
 *
 * A handle's phase descriptors carry ONE set of tracking references (xr, ur, yr, foot_pos, foot_vel, body_pos, ref_contact) that the whole
 * batch shares.  hsddp_set_references gives problems of a phase references of their own, so one handle can hold a fleet of robots at
 * different places in the world, or one gait at several commanded speeds.  Widths are those of hsddp_phase_desc_t: xr n, ur m, yr p,
 * foot_pos 12, foot_vel 12, body_pos 3, ref_contact 4; each array is [nb][h+1][width], problem-major, row-major.
 *
 * Semantics:
 *   - The first call on a phase switches it to per-problem storage: all B problems are first filled from the shared references, then
 *     problems [b0, b0+nb) take the given arrays.  Problems outside the range behave exactly as before.
 *   - Later calls overwrite problems [b0, b0+nb) only.  A NULL field keeps its current values.
 *   - src_device = 1: the arrays are device memory on the handle's device (for example torch tensors); no host staging.
 *     src_device = 0: host memory, which the caller may reuse on return.  Either way the new references are in place on return.
 *   - hsddp_reconfigure returns every phase of the new window to the shared references of its descriptors: a fleet calls
 *     hsddp_set_references again after each reconfigure.
 *   - hsddp_warm_start_phase, the ensembles and both command exports are unaffected.
 *   - HSDDP_EINVAL, with the handle unchanged: phase out of range, nb <= 0, [b0, b0+nb) outside the batch, yr given for a phase with p = 0.
 *   - Storage comes from an arena owned by the handle, grown on demand and freed by hsddp_destroy: an MPC loop that calls reconfigure and
 *     then set_references every tick makes no device allocation once warm.
 *   - fp32 handles (HSDDP_PREC_F32) keep their references in fp64 too.  Whole-body phases also keep the packed per-knot record the rollout
 *     reads (xr | ur | foot_vel | ref_contact | foot_pos - body_pos), rebuilt on the device from the new values.
 *
 * hsddp_get_references copies the references of problems [b0, b0+nb) into host arrays of the same layout (shared or per-problem alike);
 * a NULL destination skips that field.  Same HSDDP_EINVAL conditions.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.
 */
#ifndef HSDDP_REFS_H
#define HSDDP_REFS_H
#include "hsddp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_refs {          /* each [nb][h+1][width], widths as in hsddp_phase_desc_t; NULL = keep current values */
    const double *xr, *ur, *yr, *foot_pos, *foot_vel, *body_pos;
    const int *ref_contact;
} hsddp_refs_t;

int hsddp_set_references(hsddp_handle_t *h, int phase, int b0, int nb, const hsddp_refs_t *refs, int src_device);
int hsddp_get_references(hsddp_handle_t *h, int phase, int b0, int nb, double *xr, double *ur, double *yr,
                         double *foot_pos, double *foot_vel, double *body_pos, int *ref_contact);   /* host dst; NULL skips */

#ifdef __cplusplus
}
#endif
#endif
