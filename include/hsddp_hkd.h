/*
 * hsddp_hkd.h — HKD-MPC command export on top of include/hsddp.h (libhsddp_hip.so).
 *
 * HKDMPCSolver::update ends with update_foot_placement() and publish_mpc_cmd() (HKDMPC/HKDMPC.cpp:207-297), which fill hkd_command_lcmt
 * (lcmtypes/hkd_command_lcmt.lcm).  hsddp_export_hkd_commands packs that message for a range of problems of a kinodynamic handle in one
 * k_pack_hkd launch; the caller copies each row into its lcm-gen struct (LCM's big-endian wire encoding and fingerprint stay there).
 *
 * Wire layout: one row per problem of HSDDP_HKD_CMD_WORDS 32-bit words in host byte order, byte-identical to a memcpy of the packed C struct
 * with the LCM fields in declaration order and no padding.  A double takes two consecutive words, low word first (little-endian hosts).
 *
 *   words       field                          source
 *   0           int32  N_mpcsteps              n_steps (the reference publishes nsteps_between_mpc + 7 = 9; valid range 1..10)
 *   1..20       double mpc_times[10]           mpc_time + k * dt in fp64 (dt: the knot step, the reference's dt_mpc = mpc_config.timeStep)
 *   21..260     float  hkd_controls[10][24]    Ubar[s] of the phase the walk has reached
 *   261..380    float  des_body_state[10][12]  Xbar[s][0..12)
 *   381..420    int32  contacts[10][4]         the phase's contact pattern
 *   421..500    double statusTimes[10][4]      the phase's contact durations (caller-supplied status_times; zeros if NULL)
 *   501..512    float  foot_placement[12]      footholds (below)
 *   513..1952   float  feedback[10][12][12]    K[s](m, n) for m, n < 12, row-major in the message (K is column-major 24 x 24 on the device:
 *                                              feedback[k][m][n] = K[n * 24 + m])
 *   1953        float  solve_time              hsddp_get_solve_time_ms of the handle
 *
 * Walk over the knots (publish_mpc_cmd): k = 0 .. n_steps-1 with `if (s >= horizon) { s = 0; i++; }` across all phases of the window.
 * Footholds (update_foot_placement): for i = 0 .. min(n_phases - 2, 4), the first boundary where leg l goes from 0 to 1 gives
 * pf[l] = (float) Xbar_{phase i+1}[0][12 + 3l .. 15 + 3l]; a leg not found keeps the caller's current foothold pf_in (hkd_data_lcmt
 * foot_placements, HKDMPC.cpp:190-194), zeros if pf_in is NULL.
 * Deviation: rows k >= n_steps are zero (the reference keeps whatever its previous message left in the member struct).
 * K, Xbar and Ubar are fp64 in HSDDP_PREC_F32 handles too: both precisions are served, with the same fp64 -> fp32 casts.
 *
 * Conventions as in hsddp.h: 0 on success, a negative HSDDP_E* code otherwise.  Staging buffers and the step / foothold maps are kept in the
 * handle, grown on demand and freed by hsddp_destroy: a warm call makes no device allocation.
 */
#ifndef HSDDP_HKD_H
#define HSDDP_HKD_H
#include "hsddp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define HSDDP_HKD_CMD_WORDS 1954
#define HSDDP_HKD_MAX_STEPS 10
/* word offsets of the fields of one row */
#define HSDDP_HKD_OFF_N_MPCSTEPS 0
#define HSDDP_HKD_OFF_MPC_TIMES 1
#define HSDDP_HKD_OFF_CONTROLS 21
#define HSDDP_HKD_OFF_BODY_STATE 261
#define HSDDP_HKD_OFF_CONTACTS 381
#define HSDDP_HKD_OFF_STATUS_TIMES 421
#define HSDDP_HKD_OFF_FOOT_PLACEMENT 501
#define HSDDP_HKD_OFF_FEEDBACK 513
#define HSDDP_HKD_OFF_SOLVE_TIME 1953

/* rows for problems [b0, b0+nb): row i is the message of problem b0+i.  status_times: n_phases x 4 doubles shared by the batch (or NULL);
 * pf_in: nb x 12 floats, row i the current footholds of problem b0+i (or NULL).  dst_device = 1: `out` is device memory on the handle's
 * device (written directly, complete on return); 0: host memory.  HSDDP_EINVAL if a phase of the handle is not HSDDP_MODEL_HKD, n_steps is
 * outside 1..HSDDP_HKD_MAX_STEPS, the window has fewer than n_steps control knots, or [b0, b0+nb) is not inside the batch. */
int hsddp_export_hkd_commands(hsddp_handle_t *h, int b0, int nb, int n_steps, double mpc_time, double dt,
                              const double *status_times, const float *pf_in, unsigned int *out, int dst_device);
/* the nb = 1 case into host memory; bit-identical to the row of the batched call */
int hsddp_export_hkd_command(hsddp_handle_t *h, int problem, int n_steps, double mpc_time, double dt,
                             const double *status_times, const float *pf_in, unsigned int *out);

#ifdef __cplusplus
}
#endif
#endif
