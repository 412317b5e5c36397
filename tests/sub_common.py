"""Shared by tests/test_substep_host.py and tests/test_substep_gpu.py: the reference of a SUB-STEPPED closed-loop window (include/hsddp_substep.h),
the host build of the sub-stepped program (tests/_emu/sub_emu.cpp) behind numpy arguments, and the comparison against the reference.

Reference: mc_common.oracle_walk with the knot step replaced by S calls of the oracle's model probe oracle_wb_dynamics(x, u, contact, 3.1415, pi,
BG_alpha, dt / S) under the SAME u, the divergence test after each; it keeps the force of every substep, Y [B, R, n, S, 12], and the mask
`counted` [B, R, n, S] (the sample was alive when the substep began).  Policy rows come from the handle under test (mc_common.policy_of).

Tolerances.  X, U, x_final and the summaries: sim_common.compare_window, RTOL = 1e-8 x scale (a 1e-12 change of x0 grows by 66 x in X and 390 x in Y
through the 48-step window at S = 2, 3 and 4 alike, measured on the CPU).  Forces and the three float records: grf_common.force_bound.  first_slip
and n_slip EXACTLY, under grf_common's precondition, asserted: every counted stance (foot, substep) pair of the reference lies >= 1000 x the force
bound from both thresholds.  first_fall and n_sat: mc_common.compare_extra (exactly, at most one sample per case within NEAR of a threshold left out)."""
import ctypes as C
import os
import subprocess

import numpy as np

import sim_common as sc
import mc_common as mc
import grf_common as gc
from conftest import ROOT

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


def _dp(a):
    return a.ctypes.data_as(DP)


def oracle_walk_sub(pkg, oracle_lib, phases, policy, smap, x0, S, dist=None, kick=None):
    """x0: [B, R, 36]; S: substeps per control step.  Returns what mc_common.oracle_walk returns - X [B, R, n + 1, 36], U [B, R, n, 12], first_bad,
    first_fall, n_sat, sat_margin, fall_margin [B, R] - and Y [B, R, n, S, 12], counted [B, R, n, S]."""
    d = dist if dist is not None else pkg.sim.Disturbance()
    B, R = x0.shape[:2]
    n = smap.shape[1]
    X = np.zeros((B, R, n + 1, 36)); U = np.zeros((B, R, n, 12)); Y = np.zeros((B, R, n, S, 12)); counted = np.zeros((B, R, n, S), dtype=bool)
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
                z = pkg.sim.mc_normals(d.seed, d.first_problem + b, r, s) if noisy else np.zeros(48)      # numbered by the CONTROL step
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
                u = np.ascontiguousarray(u)
                h = D[p].dt / S      # one division
                for j in range(S):
                    xn = np.zeros(36); y = np.zeros(12)
                    oracle_lib.oracle_wb_dynamics(_dp(x), _dp(u), contact[p].ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi),
                                                  C.c_double(D[p].BG_alpha), C.c_double(h), _dp(xn), _dp(y))
                    Y[b, r, s, j] = y; counted[b, r, s, j] = True
                    nsq = float(xn @ xn)
                    if not (nsq <= 1e12):      # the divergence test after EVERY substep: the state from before it is kept, nothing further is done
                        first_bad[b, r] = s; alive = False
                        break
                    x = xn
                if alive and reset:
                    xi = np.zeros(36)
                    oracle_lib.oracle_wb_impact(_dp(x), contact[p].ctypes.data_as(IP), nxt[p].ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                    x = xi
            X[b, r, n] = x
            if alive:
                fall_test(n)
    for a in (X, U, Y, counted):
        a.setflags(write=False)
    return dict(X=X, U=U, Y=Y, counted=counted, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin)


def sub_margins(Y, contact, mu, fz_min, counted):
    """(min |cone|, min |fz - fz_min|) over the counted stance (foot, substep) pairs of Y [..., n, S, 12]."""
    n, S = Y.shape[-3], Y.shape[-2]
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    st = np.broadcast_to((np.asarray(contact).reshape(n, 1, 4) > 0), F.shape[:-1]) & np.asarray(counted)[..., None]
    cone = mu * F[..., 2] - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    return float(np.abs(cone[st]).min()), float(np.abs(F[..., 2][st] - fz_min).min())


def compare_records_sub(tag, pkg, rows, Y, ref, contact, mu, fz_min):
    """rows (GRF_ROW_DTYPE) and Y [B, R, n, 12] (or None) of the backend under test against the reference walk `ref` (oracle_walk_sub): forces of
    substep 0 and the three floats within the force bound, first_slip and n_slip EQUAL under the asserted margin precondition.  Returns the
    reference rows."""
    Yref = ref["Y"]
    bound = gc.force_bound(Yref)
    scale = bound / sc.RTOL
    want = pkg.sim.grf_rows_sub(Yref, contact, mu, fz_min, counted=ref["counted"])
    mcone, mfz = sub_margins(Yref, contact, mu, fz_min, ref["counted"])
    print(f"[sub] {tag}: S {Yref.shape[-2]}, mu {mu}, force scale {scale:.3e} N, force bound {bound:.3e} N, reference margins min|cone| {mcone:.3e} N, "
          f"min|fz - fz_min| {mfz:.3e} N (needed {gc.MARGIN_FACTOR * bound:.3e}), slipping samples {int((want['first_slip'] >= 0).sum())} of {want.size}, "
          f"n_slip total {int(want['n_slip'].sum())}, min fz {want['min_fz'].min():.4f} N")
    assert mcone >= gc.MARGIN_FACTOR * bound and mfz >= gc.MARGIN_FACTOR * bound, \
        f"{tag}: the reference is within {gc.MARGIN_FACTOR:.0f} x the force bound of a threshold ({mcone:.3e}, {mfz:.3e})"
    if Y is not None:
        sc.close(tag + " Y", Y, Yref[..., 0, :])
        gc.assert_swing_is_zero(tag, Y, contact)
    for f in ("min_fz", "min_cone", "max_fz"):
        sc.close(f"{tag} {f}", rows[f], want[f], scale=scale)
    assert np.array_equal(rows["first_slip"], want["first_slip"]), (tag, rows["first_slip"], want["first_slip"])
    assert np.array_equal(rows["n_slip"], want["n_slip"]), (tag, rows["n_slip"], want["n_slip"])
    return want


# ---- the host build of the sub-stepped program

def build_emu(tmpdir):
    out = os.path.join(str(tmpdir), "libhsddp_sub_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "sub_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    # the parked column of the six sub-stepped kernels: 27 / 29 doubles per lane without records, 32 / 34 with them
    assert [lib.sub_emu_park_doubles(m, g) for m, g in ((0, 0), (1, 0), (0, 1), (1, 1))] == [27, 29, 32, 34]
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, dist=None, kick=None, mu=0.0, fz_min=0.0, keep_traj=True):
    """The host build on problem b of a solved handle; x0, kick: [R, 36].  S >= 1: the SUB walk; S == 0: the walk without the switch.  dist / kick
    None: the plain walk, else the disturbed one.  mu > 0: with records.  Returns a dict of raw arrays: xf, rows, X, U, extra, g, Y."""
    nph = len(so.phases)
    D = [p["desc"] for p in so.phases]
    hor = np.array([q.horizon for q in D], dtype=np.int32); dt = np.array([q.dt for q in D]); al = np.array([q.BG_alpha for q in D])
    ct = np.array([[q.contact[l] for l in range(4)] for q in D], dtype=np.int32)
    td = np.array([[1 if (q.contact[l] == 0 and q.next_contact[l] == 1) else 0 for l in range(4)] for q in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]      # column-major 12 x 36 per knot
    ptrs = lambda arrs: (C.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n, R = smap.shape[1], x0.shape[0]
    x0 = np.ascontiguousarray(x0); smap = np.ascontiguousarray(smap, dtype=np.int32)
    xf = np.zeros((R, 36)); rows = np.zeros((R, 5)); X = np.zeros((R, n + 1, 36)); U = np.zeros((R, n, 12)); extra = np.full((R, 2), np.nan)
    g = np.full((R, 5), np.nan); Y = np.full((R, n, 12), np.nan)
    use_mc = dist is not None or kick is not None
    d = dist if dist is not None else pkg.sim.Disturbance()
    sw = np.array([d.sigma_u, d.sigma_q, d.sigma_v, d.u_max, d.fall_height])
    kick = None if kick is None else np.ascontiguousarray(kick)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.sub_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), C.c_double(mc.PSI_DYN), vp(smap), n, R, vp(x0), vp(xf), vp(rows),
                         vp(X) if keep_traj else None, vp(U) if keep_traj else None, int(S), 1 if use_mc else 0, C.c_ulonglong(d.seed), d.first_problem + b, vp(sw),
                         d.kick_step, vp(kick), vp(extra), C.c_double(mu), C.c_double(fz_min), vp(g), vp(Y) if keep_traj else None)
    assert rc == 0
    return dict(xf=xf, rows=rows, X=X, U=U, extra=extra, g=g, Y=Y)


def emu_result(pkg, outs, disturbed, records):
    """The per-problem raw outputs of emu_run stacked into the dict the library's Python layer returns (rows, x_final, X, U, extra, grf, Y)."""
    st = lambda k: np.stack([o[k] for o in outs])
    raw = st("rows")
    r = np.zeros(raw.shape[:-1], dtype=pkg._abi.SIM_ROW_DTYPE)
    for i, f in enumerate(("dev_q", "dev_v", "min_height", "max_torque", "first_bad")):
        r[f] = raw[..., i]
    res = dict(rows=r, x_final=st("xf"), X=st("X"), U=st("U"))
    if disturbed:
        ex = st("extra")
        e = np.zeros(ex.shape[:-1], dtype=pkg._abi.MC_EXTRA_DTYPE)
        e["first_fall"] = ex[..., 0]; e["n_sat"] = ex[..., 1]
        res["extra"] = e
    if records:
        graw = st("g")
        assert np.array_equal(graw[..., 3:], np.round(graw[..., 3:]))      # the counters are whole numbers in doubles
        gr = np.zeros(graw.shape[:-1], dtype=pkg._abi.GRF_ROW_DTYPE)
        for i, f in enumerate(gr.dtype.names):
            gr[f] = graw[..., i]
        res["grf"] = gr; res["Y"] = st("Y")
    return res


def compare_case(tag, pkg, res, ref, xbar, contact=None, mu=0.0, fz_min=0.0):
    """One run against its reference walk: the window, the extras of a disturbed run, the records of a run with them."""
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    if "extra" in res:
        mc.compare_extra(tag, res["extra"], ref)
    if "grf" in res:
        compare_records_sub(tag, pkg, res["grf"], res.get("Y"), ref, contact, mu, fz_min)
