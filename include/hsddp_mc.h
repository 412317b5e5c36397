/*
 * hsddp_mc.h — disturbed runs of a closed-loop simulation object (include/hsddp_sim.h): actuator noise, state-estimate noise, torque limits and
 * pushes, per sample, for Monte-Carlo robustness runs of a solved whole-body policy (libhsddp_hip.so).
 *
 * hsddp_mc_run is hsddp_sim_run with disturbances.  For problem b (global index first_problem + b), sample r, step s of the window, while the
 * sample is alive (not diverged):
 *
 *   1. push       if a kick array is given and s == kick_step:  x <- x + kick[b][r]   (36 numbers; behind a reset map where one precedes the step)
 *   2. record     x as hsddp_sim_run does (deviations, lowest height, trajectory entry s).  If fall_height > 0, x[2] < fall_height and no fall
 *                 was recorded yet: first_fall = s.  A fallen sample goes on.
 *   3. policy     on an estimate:  xh = x + e,  e[i] = sigma_q z (i < 18) / sigma_v z (i >= 18), a fresh z ~ N(0, 1) per coordinate and step;
 *                 u_cmd = Ubar + K (xh - Xbar)
 *   4. actuator   u_raw = u_cmd + sigma_u z (fresh per joint and step).  If u_max > 0: n_sat += the number of joints with |u_raw| > u_max and
 *                 u = clip(u_raw, -u_max, u_max); else u = u_raw.  max_torque and the trajectory's U entry are of the applied u.
 *   5. step and reset map as hsddp_sim_run (the impact takes no disturbance).
 *
 * Behind the last step the final state is recorded and takes the fall test with index n_steps.  A term whose sigma is 0 is skipped (no draw,
 * nothing added).  A diverged sample behaves as in hsddp_sim_run and counts no further saturations, falls or kicks.
 *
 * The noise is generated in the kernel and is a stateless function of (seed, global problem, sample, step, coordinate) alone - not of the batch,
 * the number of samples or the window length: a shard reproduces its slice, a longer window extends a shorter one, more samples extend an
 * experiment.  With draw(n), n >= 1, the n-th output of SplitMix64(seed) (state seed + n 0x9E3779B97F4A7C15 mod 2^64, two multiply-xorshift
 * rounds, (z >> 11) 2^-53), and coordinate c = 0..11 the torque of joint c, c = 12..47 the state coordinate c - 12:
 *
 *     n0 = 2 ((((first_problem + b) 65536 + r) 65536 + s) 48 + c)        (64-bit arithmetic)
 *     z  = sqrt(-2 ln(1 - draw(n0 + 1))) cos(2 pi draw(n0 + 2))           (fp64)
 *
 * cafe-mpc_amd/sim.py mc_normals states this in numpy; the uniforms of the device are bit-equal to it, the normals up to the last bits of log
 * and cos.
 *
 * Rules:
 *   - Everything hsddp_sim_run refuses is refused.  Also HSDDP_EINVAL with nothing changed: a NULL hsddp_mc_dist_t, a negative or non-finite
 *     sigma, a non-finite u_max or fall_height, first_problem < 0, kick_step outside [0, n_steps) when a kick is given, an object with
 *     n_steps > 65536 or n_samples > 65536.
 *   - The handle is left bit for bit as it was.  The buffers a disturbed run needs beyond the object's are allocated at the first disturbed run
 *     of the object and kept: later disturbed runs allocate nothing, and an object that never runs disturbed holds what it held before.
 *   - hsddp_sim_get_rows / get_traj / device_final / get_kernel_time_ms serve the last run of either kind.
 *   - With every switch off and no kick the plain kernel is launched: bit-identical to hsddp_sim_run (first_fall = -1, n_sat = 0).
 */
#ifndef HSDDP_MC_H
#define HSDDP_MC_H
#include "hsddp_sim.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsddp_mc_dist {
    unsigned long long seed;
    double sigma_u;            /* N m;   0 = off */
    double sigma_q, sigma_v;   /* state-estimate error on positions / velocities; 0 = off */
    double u_max;              /* N m;   <= 0 = off */
    double fall_height;        /* m;     <= 0 = off */
    int kick_step;             /* read only when a kick array is given: 0 <= kick_step < n_steps */
    int first_problem;         /* global index of problem 0 of this handle (shards); >= 0 */
} hsddp_mc_dist_t;
typedef struct hsddp_mc_extra { int first_fall, n_sat; } hsddp_mc_extra_t;

/* hsddp_sim_run with disturbances.  kick: [B][R][36] or NULL, host (kick_device = 0) or device memory */
int hsddp_mc_run(hsddp_sim_t *s, const double *x0, int x0_device, const hsddp_mc_dist_t *d, const double *kick, int kick_device);
/* first_fall / n_sat of problems [b0, b0+nb) of the last run; HSDDP_EINVAL if the last run of the object was not hsddp_mc_run */
int hsddp_mc_get_extra(hsddp_sim_t *s, int b0, int nb, hsddp_mc_extra_t *out);

#ifdef __cplusplus
}
#endif
#endif
