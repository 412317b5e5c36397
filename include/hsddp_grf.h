/*
 * hsddp_grf.h — ground-reaction-force records of a closed-loop simulation object (include/hsddp_sim.h, include/hsddp_mc.h; libhsddp_hip.so).
 *
 * The simulation holds the stance feet of a phase to the ground as bilateral constraints (mode 0 of the contact solve): a foot gets whatever force
 * the constraint needs, also one that pulls on the ground or lies outside the friction pyramid.  With the records switched on, a run also reports
 * what it asked of the ground.  For sample (b, r), step s of the window, phase i of that step and foot l in {FL, FR, HL, HR} with contact[l] > 0 in
 * phase i:
 *
 *     f = (fx, fy, fz)   the contact force of the step in world axes: the multiplier of the mode-0 contact solve, entries 3 l .. 3 l + 2 of
 *                        HSDDP_F_Y after a rollout - the quantity the solver constrains (c_grf, mu; MHPCConstraint.cpp:9-70) and exports
 *                        (GRF[12] of MHPC_Command_lcmt)
 *     cone = mu fz - max(|fx|, |fy|)      the friction pyramid of MHPCConstraint.cpp, in newtons
 *     the foot VIOLATES at s  iff  fz < fz_min  or  cone < 0      (both strict)
 *
 * The row of a sample is taken over the steps the sample is alive at, by the rule of max_torque: a step counts if the sample had not diverged
 * before it (the step that diverges counts; its forces are those of the kept state).  min_fz and min_cone are margins in newtons, not a required
 * friction coefficient: |ft| / fz is ill-conditioned where fz -> 0.
 *
 * With keep_traj the forces themselves are kept, Y [B][R][n_steps][12]; the three entries of a swing leg are exactly 0.  Entries behind first_bad
 * are the forces of the kept state, as U holds what the policy asks for there.  The impact solve (mode 1) takes no record.
 *
 * Forces that are not finite: the step at which a sample diverges counts, and its forces may be NaN or infinite where the state it is computed
 * from is extreme.  A NaN force violates nothing (every comparison with it is false) and the three floats ignore it (the minima and the maximum
 * are taken with fmin / fmax semantics), whereas numpy's min and max propagate it: for such a sample min_fz, min_cone and max_fz are NOT defined
 * by this header, and sim.grf_rows may differ from the device.  first_slip, n_slip and the forces in Y are as computed.
 *
 * Rules:
 *   - hsddp_grf_set(mu > 0) switches the records on with these thresholds for every later hsddp_sim_run and hsddp_mc_run of the object;
 *     mu == 0 switches them off again, and later runs launch exactly the kernels they launched before the records existed.  HSDDP_EINVAL with
 *     nothing changed: a NULL object, a negative or non-finite mu or fz_min.
 *   - The buffers are allocated by the first call that switches the records on (rows, and Y if the object was created with keep_traj) and kept:
 *     later calls and all runs allocate nothing (hsddp_debug_malloc_count).  An object that never switches them on holds what it held before.
 *   - Switching the records on changes nothing else a run returns: rows, x_final, X, U and the extras are bit-identical to the same run with
 *     the records off.  The handle is left bit for bit as it was, as by every simulation call.
 *   - hsddp_grf_get returns the records of problems [b0, b0 + nb) of the last run.  HSDDP_EINVAL: the last run of the object was made with the
 *     records off (or there was none), a bad range, rows NULL, Y non-NULL on an object without keep_traj.
 */
#ifndef HSDDP_GRF_H
#define HSDDP_GRF_H
#include "hsddp_sim.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_grf_row {
    double min_fz;    /* smallest stance fz                          (+inf if no stance foot was seen) */
    double min_cone;  /* smallest cone margin                        (+inf likewise) */
    double max_fz;    /* largest stance fz                           (-inf likewise) */
    int first_slip;   /* first step with a violating foot, else -1 */
    int n_slip;       /* number of violating (foot, step) pairs */
} hsddp_grf_row_t;    /* 32 bytes */

int hsddp_grf_set(hsddp_sim_t *s, double mu, double fz_min);
int hsddp_grf_get(hsddp_sim_t *s, int b0, int nb, hsddp_grf_row_t *rows, double *Y /* [nb][R][n_steps][12] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
