"""Shared by tests/test_plant_host.py and tests/test_plant_gpu.py: the references of closed-loop windows with a PER-SAMPLE PLANT (include/hsddp_plant.h),
the host build of the ten programs (tests/_emu/plant_emu.cpp) behind numpy arguments, and the cases.

Reference.  The oracle with link constants that can be varied (tests/_emu/plant_ref.cpp: the whole oracle plus plant_ref_set, built into a temporary
directory with the oracle's own flags - a library of its own, so the oracle the solves run on is never touched), and two restated walks:
    oracle_walk_sub_plant   sub_common.oracle_walk_sub     the bilateral walks
    oracle_walk_ter_plant   ter_common.oracle_walk_ter     the walks with terrain; with a one-cell flat map and early = 0 the walks with the contact rule alone
                                                            (tests/test_terrain_host.py holds that equality)
with three additions each: the sample's links are set before its walk, every solve is given  gain o u - damping o x[24:36]  of the state it starts from,
and the nominal links are restored at the end.  The noise numbering by (global problem, sample, step) is untouched - which is why the originals cannot
simply be called on one-sample slices.  tests/test_plant_host.py holds both restatements to the originals bit for bit at a nominal table.

Tolerances: the project's own, unchanged - sim_common.RTOL x scale on trajectories and summaries, grf_common.force_bound on forces, integers exactly, at
most one sample of a case left out for lying within MARGIN_FACTOR x bound of a decision, asserted on the reference alone (uni_common.near_samples,
mc_common.NEAR)."""
import ctypes as C
import os
import subprocess

import numpy as np

import sim_common as sc
import mc_common as mc
import sub_common as sub
import uni_common as un
import ter_common as tc
from conftest import ROOT

DP = sub.DP
IP = sub.IP
_dp = sub._dp
W_TD = tc.W_TD


def build_ref(pkg, tmpdir):
    """The oracle with plant_ref_set (tests/_emu/plant_ref.cpp), with the flags of oracle/Makefile."""
    out = os.path.join(str(tmpdir), "liboracle_plant_ref.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-shared", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "_emu", "plant_ref.cpp"), "-o", out])
    lib = pkg._abi.bind(C.CDLL(out))
    lib.plant_ref_set.argtypes = [DP, DP]; lib.plant_ref_set.restype = None
    set_links(lib, np.array(pkg._abi.PLANT_NOMINAL))
    return lib


def set_links(ref_lib, row):
    row = np.ascontiguousarray(row, dtype=np.float64)
    ref_lib.plant_ref_set(_dp(row[:10].copy()), _dp(row[10:22].copy()))


def rows_of(plant, shape):
    """The plant row of every sample: [B, R, 46]."""
    P = plant.table()
    po = np.zeros(shape, dtype=np.int64) if plant.plant_of is None else np.asarray(plant.plant_of).reshape(shape)
    return P[po]


def oracle_walk_sub_plant(pkg, ref_lib, phases, policy, smap, x0, S, plant, dist=None, kick=None):
    """sub_common.oracle_walk_sub with a plant row per sample.  Returns the same dict."""
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
    prow = rows_of(plant, (B, R))
    try:
        for b in range(B):
            for r in range(R):
                set_links(ref_lib, prow[b, r])                       # (addition 1)
                gain, damp = prow[b, r, 22:34], prow[b, r, 34:46]
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
                    h = D[p].dt / S      # one division
                    for j in range(S):
                        xn = np.zeros(36); y = np.zeros(12)
                        ue = np.ascontiguousarray(gain * u - damp * x[24:36])      # (addition 2) what the plant applies in this substep
                        ref_lib.oracle_wb_dynamics(_dp(x), _dp(ue), contact[p].ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi),
                                                   C.c_double(D[p].BG_alpha), C.c_double(h), _dp(xn), _dp(y))
                        Y[b, r, s, j] = y; counted[b, r, s, j] = True
                        nsq = float(xn @ xn)
                        if not (nsq <= 1e12):
                            first_bad[b, r] = s; alive = False
                            break
                        x = xn
                    if alive and reset:
                        xi = np.zeros(36)
                        ref_lib.oracle_wb_impact(_dp(x), contact[p].ctypes.data_as(IP), nxt[p].ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                        x = xi
                X[b, r, n] = x
                if alive:
                    fall_test(n)
    finally:
        set_links(ref_lib, np.array(pkg._abi.PLANT_NOMINAL))         # (addition 3)
    for a in (X, U, Y, counted):
        a.setflags(write=False)
    return dict(X=X, U=U, Y=Y, counted=counted, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin)


def flat_terrain(pkg):
    """The terrain under which the walk with terrain is the walk with the contact rule alone."""
    return pkg.sim.Terrain(H=np.zeros((1, 1, 1)), early=False)


def oracle_walk_ter_plant(pkg, ref_lib, phases, policy, smap, x0, S, fz_rel, z_ground, ter, plant, dist=None, kick=None, F0=None, E0=None):
    """ter_common.oracle_walk_ter with a plant row per sample (ter None: the flat one-cell map, early = 0 - the contact rule alone).  Returns the same dict."""
    ter = flat_terrain(pkg) if ter is None else ter
    d = dist if dist is not None else pkg.sim.Disturbance()
    B, R = x0.shape[:2]
    n = smap.shape[1]
    H = ter.grid()
    X = np.zeros((B, R, n + 1, 36)); U = np.zeros((B, R, n, 12)); Y = np.zeros((B, R, n, S, 12)); counted = np.zeros((B, R, n, S), dtype=bool)
    att = np.zeros((B, R, n, S, 4), dtype=bool)
    first_bad = -np.ones((B, R), dtype=np.int32); first_fall = -np.ones((B, R), dtype=np.int32); n_sat = np.zeros((B, R), dtype=np.int32)
    sat_margin = np.full((B, R), np.inf); fall_margin = np.full((B, R), np.inf)
    rows = np.zeros((B, R), dtype=pkg._abi.CONTACT_ROW_DTYPE); rows["first_release"] = -1
    trows = np.zeros((B, R), dtype=pkg._abi.TERRAIN_ROW_DTYPE); trows["first_early"] = -1
    Fend = np.zeros((B, R, 4), dtype=bool); Eend = np.zeros((B, R, 4), dtype=bool); solves = np.zeros((B, R), dtype=np.int64)
    force_margin = np.full((B, R), np.inf); kin_margin = np.full((B, R), np.inf); raw_kin = [np.inf, np.inf]
    raw_ix = [np.inf, -np.inf]; raw_iy = [np.inf, -np.inf]; cells = set(); pz_final = np.zeros((B, R, 4)); land_z = np.full((B, R, 2), np.nan)
    D = [p["desc"] for p in phases]
    contact = [np.array([dd.contact[l] for l in range(4)], dtype=np.int32) for dd in D]
    nxt = [np.array([dd.next_contact[l] for l in range(4)], dtype=np.int32) for dd in D]
    noisy = d.sigma_u > 0 or d.sigma_q > 0 or d.sigma_v > 0
    zero4 = np.zeros(4, dtype=np.int32)
    prow = rows_of(plant, (B, R))

    def foot_kin(x):
        pos = np.zeros((4, 3)); vel = np.zeros((4, 3)); J = np.zeros((4, 3, 18)); Jv = np.zeros((4, 3, 18))
        ref_lib.oracle_wb_foot_kin(_dp(x), C.c_double(mc.PSI_DYN), C.c_double(np.pi), _dp(pos), _dp(vel), _dp(J), _dp(Jv))
        return pos, vel
    try:
        for b in range(B):
            for r in range(R):
                set_links(ref_lib, prow[b, r])                       # (addition 1)
                gain, damp = prow[b, r, 22:34], prow[b, r, 34:46]
                x = x0[b, r].astype(np.float64).copy(); alive = True
                F = np.zeros(4, dtype=bool) if F0 is None else np.array(F0[b, r], dtype=bool)
                E = np.zeros(4, dtype=bool) if E0 is None else np.array(E0[b, r], dtype=bool)
                m = 0 if ter.map_of is None else int(np.asarray(ter.map_of)[b, r])
                lift = -np.inf; pen = -np.inf

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
                    Cs = contact[p] > 0
                    F = F & Cs
                    E = E & ~Cs
                    h = D[p].dt / S

                    def solve(A):
                        xn = np.zeros(36); y = np.zeros(12)
                        ue = np.ascontiguousarray(gain * u - damp * x[24:36])      # (addition 2) of the state this solve starts from
                        ref_lib.oracle_wb_dynamics(_dp(x), _dp(ue), np.ascontiguousarray(A, dtype=np.int32).ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi),
                                                   C.c_double(D[p].BG_alpha), C.c_double(h), _dp(xn), _dp(y))
                        solves[b, r] += 1
                        return xn, y
                    for j in range(S):
                        counted[b, r, s, j] = True
                        tested = (F & Cs) | ((~Cs & ~E) if ter.early else np.zeros(4, dtype=bool))
                        if tested.any():
                            pos, vel = foot_kin(x)
                            zg = z_ground + pkg.sim.terrain_height(ter, pos[:, :2], m)
                            dz = pos[:, 2] - zg; wz = vel[:, 2]
                            thr = np.where(Cs, 0.0, -ter.w_td)
                            if (F & Cs).any():
                                lift = max(lift, float(dz[F & Cs].max()))
                            T = tested & (dz <= 0.0) & (wz < thr)
                            for f in np.flatnonzero(tested):
                                wv = wz[f] - thr[f]
                                raw_kin[0] = min(raw_kin[0], abs(dz[f])); raw_kin[1] = min(raw_kin[1], abs(wv))
                                mg = min(abs(dz[f]), abs(wv)) if T[f] else max(abs(dz[f]) if dz[f] > 0.0 else 0.0, abs(wv) if wv >= 0.0 else 0.0)
                                kin_margin[b, r] = min(kin_margin[b, r], mg, tc._edge_margin(ter, H, m, pos[f, :2]))
                                ix = np.floor((pos[f, 0] - ter.x0) / ter.cx); iy = np.floor((pos[f, 1] - ter.y0) / ter.cy)
                                raw_ix[0] = min(raw_ix[0], ix); raw_ix[1] = max(raw_ix[1], ix); raw_iy[0] = min(raw_iy[0], iy); raw_iy[1] = max(raw_iy[1], iy)
                                cells.add((m, int(np.clip(iy, 0, H.shape[1] - 1)), int(np.clip(ix, 0, H.shape[2] - 1))))
                            if T.any():
                                pen = max(pen, float((-dz[T]).max()))
                                land_z[b, r] = np.nanmin([land_z[b, r, 0], pos[T, 2].min()]), np.nanmax([land_z[b, r, 1], pos[T, 2].max()])
                                xi = np.zeros(36)
                                ref_lib.oracle_wb_impact(_dp(x), zero4.ctypes.data_as(IP), T.astype(np.int32).ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                                x = xi; F = F & ~T; rows["n_land"][b, r] += int((T & Cs).sum())
                                Te = T & ~Cs
                                if Te.any():
                                    E = E | Te; trows["n_early"][b, r] += int(Te.sum())
                                    if trows["first_early"][b, r] < 0:
                                        trows["first_early"][b, r] = s
                        while True:
                            A = (Cs & ~F) | E
                            xn, y = solve(A)
                            lz = y.reshape(4, 3)[:, 2]
                            if A.any():
                                force_margin[b, r] = min(force_margin[b, r], float(np.abs(lz[A] - fz_rel).min()))
                            if not A.any() or not (lz[A].min() < fz_rel):
                                break
                            cand = np.where(A, lz, np.inf)
                            f = int(np.argmin(cand))
                            if A.sum() > 1:
                                force_margin[b, r] = min(force_margin[b, r], float(np.sort(cand)[1] - cand[f]))
                            if Cs[f]:
                                F = F.copy(); F[f] = True
                                rows["n_release"][b, r] += 1
                                if rows["first_release"][b, r] < 0:
                                    rows["first_release"][b, r] = s
                            else:
                                E = E.copy(); E[f] = False
                                trows["n_early_release"][b, r] += 1
                        Y[b, r, s, j] = y; att[b, r, s, j] = A
                        rows["n_free"][b, r] += int((F & Cs).sum()); trows["n_held"][b, r] += int(E.sum())
                        nsq = float(xn @ xn)
                        if not (nsq <= 1e12):
                            first_bad[b, r] = s; alive = False
                            break
                        x = xn
                    if alive and reset:
                        xi = np.zeros(36)
                        ref_lib.oracle_wb_impact(_dp(x), contact[p].ctypes.data_as(IP), nxt[p].ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                        x = xi
                X[b, r, n] = x
                if alive:
                    fall_test(n)
                Fend[b, r] = F; Eend[b, r] = E
                rows["free_final"][b, r] = int(sum(1 << l for l in range(4) if F[l]))
                rows["max_lift"][b, r] = lift if np.isfinite(lift) else 0.0
                trows["early_final"][b, r] = int(sum(1 << l for l in range(4) if E[l]))
                trows["max_pen"][b, r] = pen if np.isfinite(pen) else 0.0
                pz_final[b, r] = foot_kin(x)[0][:, 2] if np.isfinite(x).all() else np.nan
    finally:
        set_links(ref_lib, np.array(pkg._abi.PLANT_NOMINAL))         # (addition 3)
    for a in (X, U, Y, counted, att):
        a.setflags(write=False)
    return dict(X=X, U=U, Y=Y, counted=counted, att=att, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin,
                rows=rows, F=Fend, solves=solves, force_margin=force_margin, kin_margin=kin_margin, raw_kin=tuple(raw_kin),
                trows=trows, E=Eend, raw_ix=tuple(raw_ix), raw_iy=tuple(raw_iy), cells=cells, pz_final=pz_final, land_z=land_z)


def impact_ref(pkg, ref_lib, desc, x, row):
    """The reset map of the phase `desc` on the state x [36] with the links of `row`."""
    ct = np.array([desc.contact[l] for l in range(4)], dtype=np.int32); nx = np.array([desc.next_contact[l] for l in range(4)], dtype=np.int32)
    xi = np.zeros(36)
    try:
        set_links(ref_lib, row)
        ref_lib.oracle_wb_impact(_dp(np.ascontiguousarray(x, dtype=np.float64)), ct.ctypes.data_as(IP), nx.ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
    finally:
        set_links(ref_lib, np.array(pkg._abi.PLANT_NOMINAL))
    return xi


# ---- the host build of the ten programs

def build_emu(tmpdir):
    out = os.path.join(str(tmpdir), "libhsddp_plant_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "plant_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    # the parked column is that of the twin with records and sub-step loop: nothing of the row is parked
    assert [lib.plant_emu_park_doubles(m, f) for f in (0, 1, 2) for m in (0, 1)] == [32, 34, 39, 41, 45, 47] and lib.plant_emu_row_doubles() == 46
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, plant_rows, plant_of=None, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, map_of=None, dist=None, kick=None, mu=0.0, fz_min=0.0,
            F=None, E=None, hold=None, expect=0):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; plant_rows [n_plants, 46], plant_of None or int [R]; family "bi", "uni" or
    "ter".  Returns raw arrays (expect != 0: the return code the call must give, and None)."""
    nph, hor, dt, al, ct, td, xb, ub, kk = tc.emu_args(pkg, so, b, x0, smap)
    ptrs = lambda arrs: (C.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n, R = smap.shape[1], x0.shape[0]
    x0 = np.ascontiguousarray(x0); smap = np.ascontiguousarray(smap, dtype=np.int32)
    xf = np.zeros((R, 36)); rows = np.zeros((R, 5)); X = np.zeros((R, n + 1, 36)); U = np.zeros((R, n, 12)); extra = np.full((R, 2), np.nan)
    g = np.full((R, 5), np.nan); Y = np.full((R, n, 12), np.nan); c = np.full((R, 6), np.nan); tr = np.full((R, 6), np.nan)
    use_mc = dist is not None or kick is not None
    d = dist if dist is not None else pkg.sim.Disturbance()
    sw = np.array([d.sigma_u, d.sigma_q, d.sigma_v, d.u_max, d.fall_height])
    kick = None if kick is None else np.ascontiguousarray(kick)
    hold = None if hold is None else np.ascontiguousarray(hold, dtype=np.int32)
    mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
    P = None if plant_rows is None else np.ascontiguousarray(plant_rows, dtype=np.float64)
    po = None if plant_of is None else np.ascontiguousarray(plant_of, dtype=np.int32)
    H = None if ter is None else ter.grid()
    t = None if ter is None else ter.to_c()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.plant_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), C.c_double(mc.PSI_DYN), vp(smap), n, R, vp(x0), vp(xf), vp(rows),
                           vp(X), vp(U), int(S), 1 if use_mc else 0, C.c_ulonglong(d.seed), d.first_problem + b, vp(sw), d.kick_step, vp(kick), vp(extra),
                           C.c_double(mu), C.c_double(fz_min), vp(g), vp(Y), 0 if family == "bi" else 1, C.c_double(fz_rel), C.c_double(z_ground), vp(c), vp(F), vp(hold),
                           None if family != "ter" else C.byref(t), vp(H), vp(mo), vp(tr), vp(E), 0 if P is None else (P.shape[0] if P.ndim == 2 else 1), vp(P), vp(po))
    assert rc == expect, (rc, expect)
    return None if expect else dict(xf=xf, rows=rows, X=X, U=U, extra=extra, g=g, Y=Y, c=c, t=tr)


def host_run(lib, pkg, so, xs, smap, S, plant, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, d=None, k=None, mu=0.0):
    P = plant.table()
    po = None if plant.plant_of is None else np.asarray(plant.plant_of)
    mo = None if ter is None or ter.map_of is None else np.asarray(ter.map_of)
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, P, None if po is None else po[b], family, fz_rel, z_ground, ter, None if mo is None else mo[b], d, None if k is None else k[b], mu)
            for b in range(xs.shape[0])]
    dis = d is not None or k is not None
    if family == "bi":
        return sub.emu_result(pkg, outs, dis, mu > 0)
    res = un.emu_result(pkg, outs, dis, mu > 0)
    if family == "ter":
        res["terrain"] = tc.terrain_rows_of(pkg, np.stack([o["t"] for o in outs]))
    return res


def library_run(pkg, solver, xs, n_steps, S, plant, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer (plant None: the plant off)."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=None if family == "bi" else (fz_rel, z_ground),
                           terrain=ter if family == "ter" else None, plant=plant)


def compare_bilateral(tag, pkg, res, ref, xbar, contact, mu, fz_min=0.0):
    """One bilateral run with the plant on against oracle_walk_sub_plant.  The window, the forces and the three float records of EVERY sample (no decision
    feeds back into a bilateral walk); first_slip, n_slip, first_fall and n_sat exactly, but for the samples whose REFERENCE passes within
    MARGIN_FACTOR x the force bound of a record threshold or within mc_common.NEAR of a torque or height threshold: at most ONE per case, asserted on the
    reference before anything is compared.  (sub_common.compare_records_sub asks for that margin of every sample: the payload rows put one (foot,
    substep) pair of the plain cases at 0.8 / 0.95 of it, so the cap of one that the walks with decisions use is applied here too.)  Returns the mask."""
    import grf_common as gc
    Yref = ref["Y"]
    n, S = Yref.shape[-3], Yref.shape[-2]
    bound = gc.force_bound(Yref); scale = bound / sc.RTOL
    F = Yref.reshape(Yref.shape[:-1] + (4, 3))
    st = np.broadcast_to((np.asarray(contact).reshape(n, 1, 4) > 0), F.shape[:-1]) & np.asarray(ref["counted"])[..., None]
    cone = mu * F[..., 2] - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    margin = np.minimum(np.where(st, np.abs(cone), np.inf), np.where(st, np.abs(F[..., 2] - fz_min), np.inf)).min(axis=(-3, -2, -1))
    near = margin < gc.MARGIN_FACTOR * bound
    if "extra" in res:
        near = near | (ref["sat_margin"] < mc.NEAR) | (ref["fall_margin"] < mc.NEAR)
    print(f"[plant] {tag}: force bound {bound:.3e} N (needed margin {gc.MARGIN_FACTOR * bound:.3e}), smallest record margin {margin.min():.3e} N, two smallest per sample "
          f"{np.sort(margin.ravel())[:2]}, left out {int(near.sum())} of {near.size}")
    assert near.sum() <= 1, f"{tag}: {int(near.sum())} samples of the reference lie within the margin of a decision"
    keep = ~near
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    if "extra" in res:
        assert np.array_equal(res["extra"]["n_sat"][keep], ref["n_sat"][keep]) and np.array_equal(res["extra"]["first_fall"][keep], ref["first_fall"][keep]), tag
    want = pkg.sim.grf_rows_sub(Yref, contact, mu, fz_min, counted=ref["counted"])
    if res.get("Y") is not None:
        sc.close(tag + " Y", res["Y"], Yref[..., 0, :])
        gc.assert_swing_is_zero(tag, res["Y"], contact)
    for f in ("min_fz", "min_cone", "max_fz"):
        sc.close(f"{tag} {f}", res["grf"][f], want[f], scale=scale)
    assert np.array_equal(res["grf"]["first_slip"][keep], want["first_slip"][keep]), (tag, res["grf"]["first_slip"], want["first_slip"])
    assert np.array_equal(res["grf"]["n_slip"][keep], want["n_slip"][keep]), (tag, res["grf"]["n_slip"], want["n_slip"])
    return near


# ---- the tables and the cases, on the fixture of the contact and terrain tests (trot 4 x 12, B = 4, R = 8 around Xbar[0], 48 steps), sized on the CPU
# with the reference alone (the margins are in the docstrings of the tests that use them)

def three_rows(pkg):
    """Nominal; a 1 kg payload at (0.05, 0, 0.04); a 2 kg payload at (0.08, 0.03, 0.05) with link_scale (0.8, 1.2, 1.1) on every leg."""
    s = pkg.sim
    nom = s.Plant.nominal().rows[0]
    return np.stack([nom, s.with_trunk(nom, *s.payload_trunk(1.0, (0.05, 0.0, 0.04))), s.with_link_scale(s.with_trunk(nom, *s.payload_trunk(2.0, (0.08, 0.03, 0.05))), (0.8, 1.2, 1.1))])


def mixed_table(pkg, shape, rows=None, index=lambda b, r: b + r):
    """The three rows with plant_of[b, r] = index(b, r) mod 3, (b + r) mod 3 unless a case says otherwise."""
    po = index(np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]) % 3
    return pkg.sim.Plant(three_rows(pkg) if rows is None else rows, plant_of=po.astype(np.int32))


def gain_damping_rows(pkg, rows):
    """`rows` with the gains linspace(0.8, 1.1, 12) and b = 0.01 on the non-nominal ones."""
    out = np.array(rows, dtype=np.float64)
    for i in range(1, out.shape[0]):
        out[i] = pkg.sim.with_damping(pkg.sim.with_gain(out[i], np.linspace(0.8, 1.1, 12)), 0.01)
    return out


def assert_table_moves_the_reference(tag, ref, ref_nominal, plant):
    """Non-vacuity, on the references alone: every sample of a non-nominal row moves by more than 1e-3 in X."""
    po = np.asarray(plant.plant_of)
    nominal_row = np.array([np.array_equal(r, plant.table()[0]) for r in plant.table()])
    moved = np.abs(ref["X"] - ref_nominal["X"]).max(axis=(-2, -1))
    off = ~nominal_row[po]
    print(f"[plant] {tag}: |X - X_nominal| of the samples of a non-nominal row {moved[off].min():.3e} .. {moved[off].max():.3e}, of a nominal row {moved[~off].max() if (~off).any() else 0.0:.3e}")
    assert off.any() and (moved[off] > 1e-3).all(), (tag, moved)
    assert not moved[~off].any()


# (family, case, S, table): the bilateral walks plain (k_sim_quad_plant) and under case D's switches with gains and friction (k_sim_quad_mc_plant); the
# contact rule on the flight kick (k_sim_quad_mc0_uni_plant), under case D's noise with the roll kick (k_sim_quad_mc_uni_plant), on a partial wave and with
# the contained divergence; the block and a map per sample under noise (k_sim_quad_mc0_ter_plant, k_sim_quad_mc_ter_plant).  "mixed": plant_common.mixed_table; "mixed2": the same rows with plant_of = (2 b + r + 2) mod 3 -
# the block's early touchdowns are many close decisions: "mixed" puts TWO samples of the reference within the margin of a landing test (2.4e-7 and 3.2e-6
# against 1e-5), and so do six other index maps tried on the CPU ((b + r + 1), (b + r + 2) with the records, (b + 2 r + 0 .. 2), (2 b + r), (2 b + r + 1):
# two or three); this one leaves out one sample, for a record threshold.
CASES = [("bi", "plain", 1, "mixed"), ("bi", "plain", 3, "mixed"), ("bi", "D", 4, "gains"), ("uni", "flight", 4, "mixed"), ("uni", "roll", 4, "mixed"), ("uni", "partial", 5, "mixed"),
         ("uni", "divergence", 4, "mixed"), ("ter", "block", 4, "mixed2"), ("ter", "maps", 4, "mixed")]


def case_of(pkg, family, case, S, table, xs):
    """(x0, dist, kick, fz_rel, z_ground, terrain, Plant) of a case on the fixture's samples."""
    if family == "bi":
        d, k = (None, None) if case == "plain" else mc.cases(pkg, xs.shape[:2])["D"][:2]
        x0, fz_rel, zg, ter = xs, 0.0, 0.0, None
    elif family == "uni":
        x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs); ter = None
    else:
        x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
    pl = mixed_table(pkg, x0.shape[:2])
    if table == "mixed2":
        pl = mixed_table(pkg, x0.shape[:2], index=lambda b, r: 2 * b + r + 2)
    if table == "gains":
        pl = pkg.sim.Plant(gain_damping_rows(pkg, pl.rows), plant_of=pl.plant_of)
    return x0, d, k, fz_rel, zg, ter, pl


def reference_of(pkg, ref_lib, phases, pol, smap, family, x0, S, fz_rel, zg, ter, pl, d, k):
    if family == "bi":
        return oracle_walk_sub_plant(pkg, ref_lib, phases, pol, smap, x0, S, pl, d, k)
    return oracle_walk_ter_plant(pkg, ref_lib, phases, pol, smap, x0, S, fz_rel, zg, ter, pl, d, k)


def compare(pkg, tag, family, res, ref, xbar, contact, mu, fz_rel):
    if family == "bi":
        return compare_bilateral(tag, pkg, res, ref, xbar, contact, mu)
    if family == "uni":
        return un.compare_case(tag, pkg, res, ref, xbar, mu, 0.0, fz_rel)
    return tc.compare_case(tag, pkg, res, ref, xbar, mu, 0.0, fz_rel)


def bad_tables(pkg):
    """(rows, plant_of) pairs hsddp_plant_set refuses, for a batch of 4 x 2 samples; the first entry of each pair may be None."""
    nom = np.array(pkg._abi.PLANT_NOMINAL)
    P = np.stack([nom, nom, nom])
    po = (np.arange(8) % 3).astype(np.int32)

    def put(i, j, v):
        Q = P.copy(); Q[i, j] = v
        return Q
    bad = [(None, po), (put(0, 0, 0.0), po), (put(1, 0, -2.0), po), (put(2, 3, np.nan), po), (put(0, 45, np.inf), po), (put(1, 22, -np.inf), po), (put(0, 4, 0.0), po),
           (put(1, 5, 0.03), po), (put(2, 9, -0.01), po), (put(0, 8, 0.05), po), (put(1, 13, 0.0), po), (put(2, 21, -0.5), po), (put(0, 34, -1e-9), po)]
    for v in (-1, 3):
        q = po.copy(); q[7] = v
        bad.append((P, q))
    return P, po, bad
