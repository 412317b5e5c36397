"""Shared by tests/test_mc_host.py and tests/test_mc_gpu.py: the reference of a DISTURBED closed-loop window (include/hsddp_mc.h) and the
comparison against it.

Reference: the window walked knot by knot in numpy, per sample - policy rows (XBAR, UBAR, K) given as arrays (read from the handle under test, so
the comparison isolates the simulation from the parity of the solve), noise from sim.mc_normals, the five steps of hsddp_mc.h, the knot step by
the oracle's model probe oracle_wb_dynamics(x, u, contact, 3.1415, pi, BG_alpha, dt), the reset map by oracle_wb_impact(x, contact,
next_contact, 3.1415, pi, 1) where sim_common.step_map marks one.  With every switch off the walk agrees with sim_common.oracle_reference
(hybrid_rollout(0, MS = 0)) to 1.5e-13: test_mc_host.py::test_undisturbed_walk_is_the_oracle_rollout.

Tolerances.  X, U, x_final and the four summaries: sim_common.compare_window, RTOL = 1e-8 x scale, the project's rollout tolerance (a 1e-12 change
of x0 grows by at most 60 x through the disturbed windows used here, so round-off-level differences stay four orders below it).  first_fall and
n_sat are integers of thresholds and are compared EXACTLY, except for a sample whose REFERENCE walk comes within NEAR = 1e-6 (100 x the
trajectory bound) of a threshold - ||u_raw| - u_max| over all joints and steps, |x[2] - fall_height| over all recorded states; at most one
sample of a case may be left out that way."""
import ctypes as C

import numpy as np

import sim_common as sc

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
NEAR = 1e-6
SEED = 20241222
PSI_DYN = 3.1415


def _dp(a):
    return a.ctypes.data_as(DP)


def policy_of(handle):
    """The policy rows of a solved handle, per phase: XBAR [B, h + 1, 36], UBAR [B, h, 12], K [B, h, 12, 36]."""
    n = len(handle.phases)
    return {f: [handle.field(i, f) for i in range(n)] for f in ("XBAR", "UBAR", "K")}


def xbar_window(policy, smap):
    return sc.window(policy["XBAR"], smap, True)


def oracle_walk(pkg, oracle_lib, phases, policy, smap, x0, dist=None, kick=None):
    """x0: [B, R, 36]; dist: sim.Disturbance or None; kick: [B, R, 36] or None.  Returns dict X [B, R, n + 1, 36], U [B, R, n, 12], first_bad,
    first_fall, n_sat [B, R] and the margins sat_margin, fall_margin [B, R] (inf where the switch is off)."""
    d = dist if dist is not None else pkg.sim.Disturbance()
    B, R = x0.shape[:2]
    n = smap.shape[1]
    X = np.zeros((B, R, n + 1, 36)); U = np.zeros((B, R, n, 12))
    first_bad = -np.ones((B, R), dtype=np.int32); first_fall = -np.ones((B, R), dtype=np.int32); n_sat = np.zeros((B, R), dtype=np.int32)
    sat_margin = np.full((B, R), np.inf); fall_margin = np.full((B, R), np.inf)
    D = [p["desc"] for p in phases]
    contact = [np.array([dd.contact[l] for l in range(4)], dtype=np.int32) for dd in D]
    nxt = [np.array([dd.next_contact[l] for l in range(4)], dtype=np.int32) for dd in D]
    noisy = d.sigma_u > 0 or d.sigma_q > 0 or d.sigma_v > 0
    for b in range(B):
        for r in range(R):
            x = x0[b, r].astype(np.float64).copy(); alive = True

            def fall_test(idx):
                if d.fall_height > 0:
                    fall_margin[b, r] = min(fall_margin[b, r], abs(x[2] - d.fall_height))
                    if x[2] < d.fall_height and first_fall[b, r] < 0:
                        first_fall[b, r] = idx
            for s in range(n):
                p, k, reset = (int(v) for v in smap[:, s])
                if alive and kick is not None and s == d.kick_step:
                    x = x + kick[b, r]
                X[b, r, s] = x
                if alive:
                    fall_test(s)
                z = pkg.sim.mc_normals(d.seed, d.first_problem + b, r, s) if noisy else np.zeros(48)
                e = np.zeros(36)
                if d.sigma_q > 0:
                    e[:18] = d.sigma_q * z[12:30]
                if d.sigma_v > 0:
                    e[18:] = d.sigma_v * z[30:48]
                u = policy["UBAR"][p][b, k] + policy["K"][p][b, k] @ ((x + e) - policy["XBAR"][p][b, k])
                if d.sigma_u > 0:
                    u = u + d.sigma_u * z[:12]
                if d.u_max > 0:
                    if alive:
                        sat_margin[b, r] = min(sat_margin[b, r], float(np.abs(np.abs(u) - d.u_max).min()))
                        n_sat[b, r] += int((np.abs(u) > d.u_max).sum())
                    u = np.clip(u, -d.u_max, d.u_max)
                U[b, r, s] = u
                if not alive:
                    continue
                xn = np.zeros(36); y = np.zeros(12)
                oracle_lib.oracle_wb_dynamics(_dp(x), _dp(np.ascontiguousarray(u)), contact[p].ctypes.data_as(IP), C.c_double(PSI_DYN), C.c_double(np.pi),
                                              C.c_double(D[p].BG_alpha), C.c_double(D[p].dt), _dp(xn), _dp(y))
                nsq = float(xn @ xn)
                if not (nsq <= 1e12):      # the rollout's divergence test: the sample keeps its state and records nothing further
                    first_bad[b, r] = s; alive = False
                    continue
                x = xn
                if reset:
                    xi = np.zeros(36)
                    oracle_lib.oracle_wb_impact(_dp(x), contact[p].ctypes.data_as(IP), nxt[p].ctypes.data_as(IP), C.c_double(PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                    x = xi
            X[b, r, n] = x
            if alive:
                fall_test(n)
    return dict(X=X, U=U, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin)


def compare_extra(tag, extra, ref):
    """first_fall and n_sat exactly, but for the samples whose reference walk passes within NEAR of a threshold (at most one per case)."""
    near = (ref["sat_margin"] < NEAR) | (ref["fall_margin"] < NEAR)
    print(f"[mc] {tag}: n_sat total {int(ref['n_sat'].sum())} on {int((ref['n_sat'] > 0).sum())} samples, falls {int((ref['first_fall'] >= 0).sum())}, "
          f"nearest torque margin {ref['sat_margin'].min():.3e}, nearest height margin {ref['fall_margin'].min():.3e}, left out {int(near.sum())}")
    assert near.sum() <= 1, tag
    assert np.array_equal(extra["n_sat"][~near], ref["n_sat"][~near]), (tag, extra["n_sat"], ref["n_sat"])
    assert np.array_equal(extra["first_fall"][~near], ref["first_fall"][~near]), (tag, extra["first_fall"], ref["first_fall"])


def compare_disturbed(tag, res, ref, xbar):
    """res: rows, x_final, extra and optionally X, U of the backend under test against the oracle walk `ref`."""
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    compare_extra(tag, res["extra"], ref)


def kick_y(shape, v):
    """The push of the cases below: + v on coordinate 19 (base velocity y) of every sample."""
    k = np.zeros(tuple(shape) + (36,)); k[..., 19] = v
    return k


def cases(pkg, shape):
    """Cases A - D of the 48-step trot window: name -> (Disturbance, kick or None)."""
    Dist = pkg.sim.Disturbance
    return {
        "A": (Dist(seed=SEED, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01), None),
        "B": (Dist(seed=SEED, u_max=8.0), None),
        "C": (Dist(seed=SEED, u_max=6.0, fall_height=0.16, kick_step=10), kick_y(shape, 0.5)),
        "D": (Dist(seed=SEED, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01, u_max=8.0, fall_height=0.16, kick_step=10), kick_y(shape, 0.3)),
    }
