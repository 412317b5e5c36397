// MPC episodes (include/hsddp_episode.h): what a tick does BEHIND the walk of wb_sim.hpp - the commit of the tick into the episode's log, rows and
// states, and the reset map that is pending when the tick ends exactly on a touchdown.  The walk itself is hsddp_sim_run / hsddp_mc_run with one
// sample per problem; nothing of it is repeated here.
//
//   epi_commit   one WAVE per problem, lanes over the 36 state + 12 control coordinates: lane c copies coordinate c of the tick's trajectory into
//                the log and forms its share of the realised tracking cost; the wave sums the shares, lane 0 folds the tick's rows into the
//                episode row and decides whether the problem's episode ends.  A frozen problem (end_reason != 0) is left alone.
//   epi_impact   one lane QUAD per problem, sixteen problems per wave, as the walk: the reset map of phase `pi` applied to the episode's state -
//                wbs_contact_dynamics in mode 1 with the phase's touchdown set and damping 0, the call of wbs_walk's phase boundary - and the state
//                handed to the solver.  Launched only when the host sees the pending map (once per touchdown, not per step).
//
//   epi_latency  (include/hsddp_latency.h) one WAVE per (problem, step) of n_exec + D steps, lanes over the 258 sixteen-byte pairs of a policy row: a
//                step below n_exec composes the row the walk applies there - from the previous tick's stash if the step is stale for the problem,
//                else from the handle - and a step from n_exec on writes the handle's row into the next stash.  A pure copy: no LDS, no atomics.
//
// All three are templates over the lane policy so that tests/_emu/episode_emu.cpp builds them for the host (EpiWaveH: the 64 lanes one after the other;
// QH: the four lanes of a quad together).  cafe-mpc_amd/episode.py fold_rows is the definition of the commit.
#pragma once
#include "wb_sim.hpp"
#include "latency_plan.hpp"

namespace hs {

// hsddp_episode_row_t as the device keeps it (the same 96 bytes: hsddp_episode_get_rows copies them out)
struct EpiRow {
    double dev_q, dev_v, min_height, max_torque, min_fz, min_cone, max_fz, track_cost;
    int n_sat, n_slip, first_slip, steps, bad_solves, end_reason, end_step, pad;
};
static_assert(sizeof(EpiRow) == 96, "EpiRow mirrors hsddp_episode_row_t");

struct EpiCommitArgs {
    int n_exec, tick, max_ticks, handoff;      // handoff 1: no reset map is pending, the commit hands the state to the solver itself
    const int* map;                            // [3][n_exec] step -> phase, knot, reset map behind the step (the simulation object's)
    const double *simX, *simU, *simY;          // the tick's trajectory [B][n_exec + 1][36], [B][n_exec][12]; forces [B][n_exec][12] or null
    const double *fin, *sim_rows;              // final states [B][36]; [B][SIM_ROW]
    const double *extra, *grf_rows;            // [B][2] first_fall | n_sat of a disturbed walk, else null; [B][SIM_GRF_ROW] with the force records on, else null
    const ProbState* st;                       // the handle's per-problem solver state (status of the last solve)
    EpiRow* rows; double *state, *x0;          // [B]; the episode's states [B][36]; the handle's initial condition [B][36]
    double *logX, *logU, *logY;                // [B][max_ticks n_exec + 1][36], [B][max_ticks n_exec][12] twice; all null without a log
};

#ifdef HS_HOST_EMU
struct EpiWaveH {      // host: the lanes of the wave one after the other, the sum in the order of the device's butterfly
    template <class F> static void each(F f) { for (int l = 0; l < 64; l++) f(l); }
    template <class F> static double sum(F f) {
        double v[64];
        for (int l = 0; l < 64; l++) v[l] = f(l);
        for (int o = 32; o; o >>= 1) for (int l = 0; l < o; l++) v[l] = v[l] + v[l + o];
        return v[0];
    }
};
#else
struct EpiWaveD {
    template <class F> static HD void each(F f) { f((int)threadIdx.x); }
    template <class F> static HD double sum(F f) {
        double v = f((int)threadIdx.x);
        _Pragma("unroll") for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
        return v;
    }
};
#endif

template <class W> HD void epi_commit(PhaseC* ph, const EpiCommitArgs& a, int b) {
    EpiRow* const row = a.rows + b;
    if (row->end_reason != 0) return;      // frozen: nothing more is logged, folded or handed over (the whole wave leaves)
    const int n = a.n_exec;
    const size_t g = (size_t)b, sx = (size_t)(n + 1) * 36, su = (size_t)n * 12, steps = (size_t)a.max_ticks * n;
    const size_t lx = (g * (steps + 1) + (size_t)a.tick * n) * 36, lu = (g * steps + (size_t)a.tick * n) * 12;
    // how the tick ended, in every lane alike
    const int fb = (int)a.sim_rows[g * SIM_ROW + 4], ff = a.extra != nullptr ? (int)a.extra[g * 2] : -1;
    int reason = 0, estep = -1;
    if (ff >= 0 && (fb < 0 || ff <= fb)) { reason = 2; estep = ff; }
    else if (fb >= 0) { reason = 1; estep = fb; }
    const double cost = W::sum([&](int l) {
        double c = 0.0;
        if (l >= 48) return c;
        for (int s = 0; s < n; s++) {
            PhaseC& P = ph[wbs_uniform(a.map[s])];
            const HS_GLOBAL double* rr = P.rref + ref_row(P, b, a.map[n + s]) * 80;      // xr | ur | ... of the knot: the problem's own row with per-problem references
            if (l < 36) {
                const double x = a.simX[g * sx + (size_t)s * 36 + l], d = x - rr[l];
                if (a.logX != nullptr) a.logX[lx + (size_t)s * 36 + l] = x;
                c += 0.5 * P.q[l] * d * d;
            } else {
                const int j = l - 36;
                const double u = a.simU[g * su + (size_t)s * 12 + j], d = u - rr[36 + j];
                if (a.logU != nullptr) a.logU[lu + (size_t)s * 12 + j] = u;
                if (a.logY != nullptr && a.simY != nullptr) a.logY[lu + (size_t)s * 12 + j] = a.simY[g * su + (size_t)s * 12 + j];
                c += 0.5 * P.r[j] * d * d;
            }
        }
        if (l < 36) {
            const double xf = a.fin[g * 36 + l];
            if (a.logX != nullptr) a.logX[lx + (size_t)n * 36 + l] = a.simX[g * sx + (size_t)n * 36 + l];
            a.state[g * 36 + l] = xf;
            if (reason == 0 && a.handoff) a.x0[g * 36 + l] = xf;
        }
        return c;
    });
    W::each([&](int l) {
        if (l != 0) return;
        const double* r = a.sim_rows + g * SIM_ROW;
        const int base = a.tick * n;
        row->dev_q = fmax(row->dev_q, r[0]); row->dev_v = fmax(row->dev_v, r[1]); row->min_height = fmin(row->min_height, r[2]); row->max_torque = fmax(row->max_torque, r[3]);
        if (a.extra != nullptr) row->n_sat += (int)a.extra[g * 2 + 1];
        if (a.grf_rows != nullptr) {
            const double* q = a.grf_rows + g * SIM_GRF_ROW;
            row->min_fz = fmin(row->min_fz, q[0]); row->min_cone = fmin(row->min_cone, q[1]); row->max_fz = fmax(row->max_fz, q[2]);
            if (row->first_slip < 0 && (int)q[3] >= 0) row->first_slip = base + (int)q[3];
            row->n_slip += (int)q[4];
        }
        row->steps += n;
        if (a.st[b].status == 1) row->bad_solves += 1;
        row->track_cost += cost;
        if (reason != 0) { row->end_reason = reason; row->end_step = base + estep; }
    });
}

// The pending reset map of phase `pi` on the state of problem g (lane = leg).  Positions stay, velocities jump; the state goes back to the episode
// and into the handle's initial condition.  A frozen problem's quad computes with the others (the cross-lane steps need every lane) and stores nothing.
template <class Q> HD void epi_impact(PhaseC* ph, const ModelDev& md, int pi, size_t g, const EpiRow* rows, double* state, double* x0) {
    using S = typename Q::S;
    PhaseC& P = ph[pi];
    S qb[6], vb[6], ql[3], vl[3], ul[3], ob[6]; V3<S> ol;
    _Pragma("unroll") for (int i = 0; i < 6; i++) { qb[i] = Q::ld(state, g * 36 + i, 0); vb[i] = Q::ld(state, g * 36 + 18 + i, 0); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { ql[j] = Q::ld(state, g * 36 + 6 + j, 3); vl[j] = Q::ld(state, g * 36 + 24 + j, 3); ul[j] = S(0.0); }
    const int cm_td = (P.td[0] ? 1 : 0) | (P.td[1] ? 2 : 0) | (P.td[2] ? 4 : 0) | (P.td[3] ? 8 : 0);
    wbs_contact_dynamics<Q>(md, cm_td, 1, 0.0, P.bg_alpha, qb, vb, ql, vl, ul, ob, ol);
    if (rows[g].end_reason != 0) return;
    const S o3[3] = {ol.x, ol.y, ol.z};
    _Pragma("unroll") for (int i = 0; i < 6; i++) { Q::st0(state, g * 36 + 18 + i, ob[i]); Q::st0(x0, g * 36 + i, qb[i]); Q::st0(x0, g * 36 + 18 + i, ob[i]); }
    _Pragma("unroll") for (int j = 0; j < 3; j++) { Q::st(state, g * 36 + 24 + j, 3, o3[j]); Q::st(x0, g * 36 + 6 + j, 3, ql[j]); Q::st(x0, g * 36 + 24 + j, 3, o3[j]); }
}

// ---- policy latency.  The effective rows live step-major - Xe [n_exec][B][2][36], Ue [n_exec][B][12], Ke [n_exec][B][432] - so that descriptor s of the
// table the walk is sent to (sim_host.hpp: a copy of the step's phase with h = 1 and Xbar, Ubar, K at slice s) makes the walk's own indexing,
// (b (h+1) + k) 36, (b h + k) 12 and (b h + k) 432 with k = 0, land on problem b's row.  A stash row is the LAT_ROW doubles in one piece.
// Every part of every row starts at a multiple of 16 bytes (288, 96, 3456 and 4128 bytes a row; the handle's arrays are aligned to 256), so a lane
// moves sixteen bytes at a time and a wave-instruction covers 1 KiB of one row.
typedef double EpiPair __attribute__((vector_size(16)));      // (a vector type, not a struct: its copies are values in registers, one dwordx4 each way)
struct EpiLatArgs {
    int n_exec, D, B, valid;                   // executed steps; largest delay; problems; 1: `prev` holds the rows the previous tick stashed
    const int* map;                            // [3][n_exec + D] step -> phase, knot over n_exec + D steps of the CURRENT window (latency_plan.hpp: long_map)
    const int* delay; int* n_stale;            // [B] delay of the problem in steps; stale steps executed while alive
    const EpiRow* rows;                        // [B] the episode rows (end_reason: a frozen problem counts nothing)
    const double* prev; double* next;          // the stashes [B][D][LAT_ROW]: read / written this tick
    double *Xe, *Ue, *Ke;                      // the effective rows, as above
};

// 258 pairs of a row from (sx | su | sk) to (dx | du | dk): 36 + 6 + 216.  Pair i of the row is lane i's in round 0 - the only round that meets all
// three parts: the lane selects its addresses, nothing branches - and pairs 64 .. 255 are K's in rounds 1 to 3; lanes 0 and 1 take the last two.  The
// four loads of the full rounds are issued before the first store.
HD void epi_lat_copy(int l, const HS_GLOBAL EpiPair* sx, const HS_GLOBAL EpiPair* su, const HS_GLOBAL EpiPair* sk, HS_GLOBAL EpiPair* dx, HS_GLOBAL EpiPair* du,
                     HS_GLOBAL EpiPair* dk) {
    const HS_GLOBAL EpiPair* const s0 = l < 36 ? sx + l : l < 42 ? su + (l - 36) : sk + (l - 42);
    HS_GLOBAL EpiPair* const d0 = l < 36 ? dx + l : l < 42 ? du + (l - 36) : dk + (l - 42);
    const EpiPair v0 = *s0, v1 = sk[l + 22], v2 = sk[l + 86], v3 = sk[l + 150];
    *d0 = v0; dk[l + 22] = v1; dk[l + 86] = v2; dk[l + 150] = v3;
    if (l < 2) dk[l + 214] = sk[l + 214];
}

template <class W> HD void epi_latency(PhaseC* ph, const EpiLatArgs& a, int b, int s) {
    const int L = a.n_exec + a.D;
    const size_t g = (size_t)b;
    const int d = wbs_uniform(HS_AS_CONST(int, a.delay)[b]);
    const bool stale = s < a.n_exec && a.valid != 0 && s < d;      // the same in every lane: a scalar branch
    HS_GLOBAL EpiPair *dx, *du, *dk;
    if (s < a.n_exec) {
        const size_t o = (size_t)s * a.B + g;
        dx = (HS_GLOBAL EpiPair*)(a.Xe + o * 72); du = (HS_GLOBAL EpiPair*)(a.Ue + o * 12); dk = (HS_GLOBAL EpiPair*)(a.Ke + o * 432);
    } else {
        double* const row = a.next + (g * a.D + (size_t)(s - a.n_exec)) * LAT_ROW;
        dx = (HS_GLOBAL EpiPair*)(row + LAT_OX); du = (HS_GLOBAL EpiPair*)(row + LAT_OU); dk = (HS_GLOBAL EpiPair*)(row + LAT_OK);
    }
    const HS_GLOBAL EpiPair *sx, *su, *sk;
    if (stale) {
        const double* const row = a.prev + (g * a.D + (size_t)s) * LAT_ROW;
        sx = (const HS_GLOBAL EpiPair*)(row + LAT_OX); su = (const HS_GLOBAL EpiPair*)(row + LAT_OU); sk = (const HS_GLOBAL EpiPair*)(row + LAT_OK);
    } else {
        PhaseC& P = ph[wbs_uniform(HS_AS_CONST(int, a.map)[s])];
        const int k = wbs_uniform(HS_AS_CONST(int, a.map)[L + s]), h = P.h;
        sx = (const HS_GLOBAL EpiPair*)(P.Xbar + (g * (h + 1) + k) * 36); su = (const HS_GLOBAL EpiPair*)(P.Ubar + (g * h + k) * 12);
        sk = (const HS_GLOBAL EpiPair*)(P.K + (g * h + k) * 432);
    }
    W::each([&](int l) { epi_lat_copy(l, sx, su, sk, dx, du, dk); });
    if (s == 0) W::each([&](int l) {      // the problem's counter: the stale steps of this tick, if it is alive at its start
        if (l == 0 && a.valid != 0 && a.rows[b].end_reason == 0) a.n_stale[b] += d < a.n_exec ? d : a.n_exec;
    });
}

#ifndef HS_HOST_EMU
// k_episode_latency and its launcher: hsddp_lat.hip, a translation unit of its own like the walks beyond the first six, so that the code object of
// hsddp_hip.hip and the list `make resources` prints stay what they were.  grid = min(B (n_exec + D), LAT_MAX_WAVES) waves: 32 waves for each of the 256
// CUs; beyond that a launch only queues workgroups.
constexpr int LAT_MAX_WAVES = 8192;
void epi_latency_launch(hipStream_t stream, unsigned grid, const PhaseDev* ph, const EpiLatArgs& a);
#endif
#if !defined(HS_HOST_EMU) && !defined(HS_EPISODE_BODIES_ONLY)      // (HS_EPISODE_BODIES_ONLY: hsddp_lat.hip takes the programs above and none of the kernels below)
// grid = B waves
__global__ void __launch_bounds__(64) k_episode_commit(const PhaseDev* ph_, EpiCommitArgs a) { epi_commit<EpiWaveD>((PhaseC*)ph_, a, (int)blockIdx.x); }
// grid = ceil(B / 16) waves of sixteen quads, compiled for the register budget of the walk (the contact solve is the same code)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SIM_WPE, SIM_WPE)))
k_episode_impact(const PhaseDev* ph_, ModelDev md, int pi, int total, const EpiRow* rows, double* state, double* x0) {
    const int g = blockIdx.x * 16 + (threadIdx.x >> 2);
    if (g >= total) return;      // (a quad leaves or stays as a whole)
    epi_impact<QS>((PhaseC*)ph_, md, pi, (size_t)g, rows, state, x0);
}
#endif

}  // namespace hs
