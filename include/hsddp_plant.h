/*
 * hsddp_plant.h — per-sample plant-model mismatch in a closed-loop simulation object (include/hsddp_sim.h, include/hsddp_mc.h, include/hsddp_grf.h,
 * include/hsddp_substep.h, include/hsddp_contact.h, include/hsddp_terrain.h, include/hsddp_episode.h; libhsddp_hip.so).
 *
 * Without this header every run simulates the robot the planner believes in: a 3.3 kg trunk with its inertia, the three link inertias per leg, and
 * torque applied exactly as commanded.  This header gives a simulation object a TABLE of plant rows and an index per sample, so that a Monte-Carlo run
 * can vary the robot itself - a payload on the trunk, a mis-identified link, a motor that delivers 90 % of its command, joint friction - and an episode
 * can run MPC against a robot that is persistently different from the model.
 *
 * The row, HSDDP_PLANT_ROW = 46 doubles.  Joints are leg-major (FL abad, hip, knee, FR, HL, HR), the order of u.
 *    0        trunk mass                        replaces 3.3
 *    1 ..  3  trunk CoM, trunk axes             replaces (0, 0, 0)
 *    4 ..  9  trunk inertia about its CoM       xx, xy, xz, yy, yz, zz; replaces 0.011253, 0, 0, 0.036203, 0, 0.042673
 *   10 .. 21  link_scale                        mass and CoM inertia of that joint's link are multiplied by it; CoM and geometry are unchanged
 *   22 .. 33  tau_gain                          applied torque gain per joint
 *   34 .. 45  damping                           viscous friction b, N m s / rad
 * The nominal row is (3.3, 0, 0, 0, 0.011253, 0, 0, 0.036203, 0, 0.042673, twelve ones, twelve ones, twelve zeros).
 *
 * Semantics.  plant_of[b][r] names the row of sample r of problem b (NULL: row 0 for every sample).
 *   - Every contact solve of the walk (forward dynamics and impacts alike: the reset map of a phase, early and unilateral landings, the pending reset
 *     map of an episode) uses the row's inertias: in the composite inertias, in the whole-robot sum, in the trunk's own bias force and in the per-link
 *     bias forces.  The kinematics - link lengths, joint placements - stay the planner's.
 *   - In every substep the torque that enters the dynamics is  tau = tau_gain o u_cmd - damping o qdot_leg  with qdot_leg of the state the solve is
 *     given: the state the substep starts from, after the landing impact if the substep has one.  u_cmd is what it was: policy plus noise, clipped once per control step and held over the substeps.  U, max_torque and n_sat go on
 *     recording u_cmd: gain and friction are the plant's secret.  Impacts take no torque.
 *   - Force records, the release and landing rules and the terrain are unchanged in form; they see the forces the mismatched plant produces.  There is
 *     no new per-sample record: the existing rows show the effect.
 *
 * The friction is EXPLICIT: it is evaluated at the start of a substep and held over it, like every other term of the forward-Euler step.  Against the
 * small reflected inertia of a leg joint this is stiff: the step is stable only while b h / I_joint < 2, h = dt / S.  On the trot fixture of the tests
 * (dt = 10 ms) b = 0.05 rings visibly at S = 2 and b = 0.2 blows up; use b <= 0.01 with S >= 2, or more substeps.  Implicit friction is out of scope.
 *
 * Rules:
 *   - HSDDP_EINVAL with nothing changed: a NULL sim; and for on != 0 a NULL P, n_plants outside 1 .. 65536, a non-finite entry, a trunk mass <= 0, a
 *     trunk inertia whose leading minors are not all > 0, a link_scale <= 0, a damping < 0, a plant_of entry outside [0, n_plants).
 *     HSDDP_ENOTSUP: on != 0 for an fp32 handle.  on = 0 ignores the rest.
 *   - P and plant_of are host pointers; the call copies them.
 *   - Dormancy: with the plant off exactly the kernels of the headers above are launched and every run is bit-identical to one before this header
 *     existed.  With it on, the walk of the family the other switches select (terrain first, then unilateral contact, then the rest) runs in its _plant
 *     twin, which always carries the sub-step loop and the force records (into a buffer of its own while hsddp_grf_set has them off).
 *   - Only a set call may allocate (the first one, and when the table grows); runs never allocate (hsddp_debug_malloc_count).  The handle is left bit
 *     for bit as it was.
 *   - hsddp_plant_get_params reads back what later runs use (on = 0, n_plants = 0 on a fresh object); hsddp_plant_get_table copies rows
 *     [p0, p0 + np) of the table back (HSDDP_EINVAL for a range outside it or a NULL argument).
 *   - hsddp_episode_sim(e) is accepted.  There n_samples is 1, so each robot has its plant for the whole episode; the table survives hsddp_reconfigure
 *     and hsddp_episode_reset.
 *
 * Out of scope: changed link lengths or joint placements; Coulomb friction; implicit friction; motor dynamics and delay; a solver that knows the plant;
 * fp32 handles; tables that already live in device memory; sliding ground friction.
 */
#ifndef HSDDP_PLANT_H
#define HSDDP_PLANT_H
#include "hsddp_terrain.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HSDDP_PLANT_ROW 46
#define HSDDP_PLANT_MAX 65536

int hsddp_plant_set(hsddp_sim_t *s, int on, int n_plants, const double *P /* [n_plants][HSDDP_PLANT_ROW] */, const int *plant_of /* [batch][n_samples] or NULL: row 0 */);
int hsddp_plant_get_params(hsddp_sim_t *s, int *on, int *n_plants);
int hsddp_plant_get_table(hsddp_sim_t *s, int p0, int np, double *P);

#ifdef __cplusplus
}
#endif
#endif
