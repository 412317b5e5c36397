"""The ONE reference of the closed-loop simulation walks, and the plumbing of their host builds.  The *_common.py modules keep their names for the
walk (mc_common.oracle_walk ... fric_common.oracle_walk_fric): each is a few lines around reference_walk below.  A new simulation feature extends
reference_walk by an argument; it does not copy it.

The walk.  Per sample, in numpy on the oracle's probes only: policy rows (XBAR, UBAR, K) given as arrays (mc_common.policy_of: read from the handle
under test, so a comparison isolates the simulation from the parity of the solve), noise from sim.mc_normals numbered by (global problem, sample,
CONTROL step) - which is why a walk cannot be composed from one-sample slices and the (problem, sample) loops are outermost.  The rules, in the
order of the headers:
  hsddp_mc.h        kick, fall test, noisy feedback, torque limit; the knot step by oracle_wb_dynamics(x, u, contact, psi, pi, BG_alpha, h), the
                    divergence test |x_next|^2 <= 1e12 (a failing sample keeps its state and records nothing further), the scheduled reset map by
                    oracle_wb_impact(x, contact, next_contact, psi, pi, 1) where sim_common.step_map marks one
  hsddp_substep.h   S solves of h = dt / S (one division per control step) under the SAME u, the divergence test after each; Y and `counted` per substep
  hsddp_contact.h   contact = (fz_rel, z_ground): F <- F n C at a phase change; a released foot lands (p_z <= z_g and w_z < 0, oracle_wb_foot_kin)
                    through oracle_wb_impact(x, 0, T); every solve runs on the attached feet A and is repeated without the foot of smallest
                    lambda_z while that is below fz_rel.  Y and att are those of a substep's LAST solve
  hsddp_terrain.h   z_g from sim.terrain_height; with ter.early a swing foot lands early (w_z < -w_td) into E, A = (C \\ F) u E, E <- E \\ C
  hsddp_plant.h     the sample's links set before its walk (plant_ref_set of tests/_emu/plant_ref.cpp) and restored at the end; every solve is given
                    gain o u - damping o x[24:36] of the state it starts from
  hsddp_friction.h  every solve is fric_ref_dynamics of tests/_emu/fric_ref.cpp on (A, Sl, f_t): a sliding foot gets the kinetic force against its
                    tangential velocity or re-sticks below v_stick; after the lift-off test a sticking foot outside its cone (mu_s) starts to slide
A feature that is off contributes no call and no arithmetic."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
PSI_DYN = 3.1415

KEYS_MC = ("X", "U", "first_bad", "first_fall", "n_sat", "sat_margin", "fall_margin")
KEYS_SUB = KEYS_MC + ("Y", "counted")
KEYS_UNI = KEYS_SUB + ("att", "rows", "F", "solves", "force_margin", "kin_margin", "raw_kin")
KEYS_TER = KEYS_UNI + ("trows", "E", "raw_ix", "raw_iy", "cells", "pz_final", "land_z")
KEYS_FRIC = KEYS_UNI + ("trows", "E", "frows", "Sl", "NF", "slide", "onset_margin", "which_margin", "stick_margin", "events")
READ_ONLY = ("X", "U", "Y", "counted", "att", "slide")


def _dp(a):
    return a.ctypes.data_as(DP)


def _ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(IP)


def pick(walk, keys, read_only=READ_ONLY):
    """The entries `keys` of a walk's dict, the trajectories among them read-only."""
    for k in keys:
        if k in read_only:
            walk[k].setflags(write=False)
    return {k: walk[k] for k in keys}


def set_links(ref_lib, row):
    row = np.ascontiguousarray(row, dtype=np.float64)
    ref_lib.plant_ref_set(_dp(row[:10].copy()), _dp(row[10:22].copy()))


def plant_rows(plant, shape):
    """The plant row of every sample: [B, R, 46]."""
    po = np.zeros(shape, dtype=np.int64) if plant.plant_of is None else np.asarray(plant.plant_of).reshape(shape)
    return plant.table()[po]


def friction_table(fric, shape):
    """(mu_s, mu_k) of every sample: two arrays [B, R]."""
    mu = fric.table()
    mo = np.zeros(shape, dtype=np.int64) if fric.mu_of is None else np.asarray(fric.mu_of).reshape(shape)
    return mu[mo, 0], mu[mo, 1]


def edge_margin(ter, H, m, p):
    """Distance of the point p (x, y) to the nearest cell edge behind which map m holds another height (inf if there is none)."""
    fx, fy = (p[0] - ter.x0) / ter.cx, (p[1] - ter.y0) / ter.cy
    ix, iy = np.floor(fx), np.floor(fy)
    h = lambda i, j: H[m, int(min(max(j, 0), H.shape[1] - 1)), int(min(max(i, 0), H.shape[2] - 1))]      # (outside the grid the edge cell holds)
    out = np.inf
    if h(ix - 1, iy) != h(ix, iy):
        out = min(out, (fx - ix) * ter.cx)
    if h(ix + 1, iy) != h(ix, iy):
        out = min(out, (ix + 1 - fx) * ter.cx)
    if h(ix, iy - 1) != h(ix, iy):
        out = min(out, (fy - iy) * ter.cy)
    if h(ix, iy + 1) != h(ix, iy):
        out = min(out, (iy + 1 - fy) * ter.cy)
    return out


def reference_walk(pkg, lib, phases, policy, smap, x0, S=1, contact=None, ter=None, plant=None, fric=None, dist=None, kick=None,
                   F0=None, E0=None, Sl0=None, NF0=None, psi_dyn=PSI_DYN):
    """x0, kick: [B, R, 36]; S: substeps per control step; contact: None (the bilateral walk: one solve per substep on the scheduled feet) or
    (fz_rel, z_ground); ter: sim.Terrain or None (with the contact rule on: the flat one-cell map without early touchdown); plant: sim.Plant or None;
    fric: sim.Friction or None; dist: sim.Disturbance or None; F0, E0, Sl0: None or bool [B, R, 4], NF0: None or float [B, R, 4] - the sets a tick hands
    over; lib: the library the probes are called on (the oracle, or the build that carries plant_ref_set or fric_ref_dynamics).

    Returns a dict (pick() cuts it to what a feature's tests see):
      X [B, R, n + 1, 36], U [B, R, n, 12], first_bad, first_fall, n_sat [B, R]; sat_margin, fall_margin [B, R] (inf where the switch is off)
      Y [B, R, n, S, 12] of every substep's last solve, counted [B, R, n, S] (the sample was alive when the substep began)
      att [B, R, n, S, 4] (the set that solve ran on, the feet of E too), rows (CONTACT_ROW_DTYPE [B, R]), F [B, R, 4] at the end, solves [B, R],
        force_margin, kin_margin [B, R] (the margins of the decisions: uni_common, ter_common, fric_common), raw_kin (smallest |p_z - z_g|, |w_z|)
      trows (TERRAIN_ROW_DTYPE), E at the end, raw_ix / raw_iy (smallest and largest raw cell index of a tested foot), cells (the set of (m, iy, ix) a
        tested foot read), pz_final [B, R, 4] (foot heights of the final state), land_z [B, R, 2] (lowest, highest p_z of a landing foot; NaN: none)
      frows (FRICTION_ROW_DTYPE), Sl and NF at the end, slide [B, R, n, S, 4] (the sliding set of every substep's last solve), onset_margin,
        which_margin, stick_margin [B, R] (folded into force_margin and kin_margin when friction is on), events: per sample a list of (step,
        substep, kind, leg), kind in onset / kinetic (the solve applied the kinetic force on the foot's non-fresh branch) / restick /
        release_sliding / phase_in_sl / slide_e (a foot of E in Sl at a substep's end)."""
    sim, abi = pkg.sim, pkg._abi
    uni = contact is not None
    assert uni or (ter is None and fric is None and F0 is None and E0 is None), "terrain and friction act through the contact rule"
    assert fric is not None or (Sl0 is None and NF0 is None)
    assert plant is None or fric is None, "no build of the oracle carries both plant_ref_set and fric_ref_dynamics"
    d = dist if dist is not None else sim.Disturbance()
    noisy = d.sigma_u > 0 or d.sigma_q > 0 or d.sigma_v > 0
    fz_rel, z_ground = contact if uni else (None, None)
    if uni and ter is None:
        ter = sim.Terrain(H=np.zeros((1, 1, 1)), early=False)
    H = ter.grid() if uni else None
    B, R = x0.shape[:2]
    n = smap.shape[1]
    D = [p["desc"] for p in phases]
    sched = [np.array([q.contact[l] for l in range(4)], dtype=np.int32) for q in D]
    sched_next = [np.array([q.next_contact[l] for l in range(4)], dtype=np.int32) for q in D]
    prow = plant_rows(plant, (B, R)) if plant is not None else None
    MUS, MUK = friction_table(fric, (B, R)) if fric is not None else (None, None)
    psi, pi = C.c_double(psi_dyn), C.c_double(np.pi)

    X = np.zeros((B, R, n + 1, 36)); U = np.zeros((B, R, n, 12)); Y = np.zeros((B, R, n, S, 12)); counted = np.zeros((B, R, n, S), dtype=bool)
    att = np.zeros((B, R, n, S, 4), dtype=bool); slide = np.zeros((B, R, n, S, 4), dtype=bool)
    first_bad = -np.ones((B, R), dtype=np.int32); first_fall = -np.ones((B, R), dtype=np.int32); n_sat = np.zeros((B, R), dtype=np.int32)
    sat_margin = np.full((B, R), np.inf); fall_margin = np.full((B, R), np.inf)
    rows = np.zeros((B, R), dtype=abi.CONTACT_ROW_DTYPE); rows["first_release"] = -1
    trows = np.zeros((B, R), dtype=abi.TERRAIN_ROW_DTYPE); trows["first_early"] = -1
    frows = np.zeros((B, R), dtype=abi.FRICTION_ROW_DTYPE); frows["first_slide"] = -1
    Fend = np.zeros((B, R, 4), dtype=bool); Eend = np.zeros((B, R, 4), dtype=bool); Slend = np.zeros((B, R, 4), dtype=bool); NFend = np.zeros((B, R, 4))
    solves = np.zeros((B, R), dtype=np.int64)
    force_margin = np.full((B, R), np.inf); kin_margin = np.full((B, R), np.inf); raw_kin = [np.inf, np.inf]
    onset_margin = np.full((B, R), np.inf); which_margin = np.full((B, R), np.inf); stick_margin = np.full((B, R), np.inf)
    raw_ix = [np.inf, -np.inf]; raw_iy = [np.inf, -np.inf]; cells = set(); pz_final = np.zeros((B, R, 4)); land_z = np.full((B, R, 2), np.nan)
    events = [[[] for _ in range(R)] for _ in range(B)]
    bits = lambda v: int(sum(1 << l for l in range(4) if v[l]))

    def foot_kin(x):
        pos = np.zeros((4, 3)); vel = np.zeros((4, 3)); J = np.zeros((4, 3, 18)); Jv = np.zeros((4, 3, 18))
        lib.oracle_wb_foot_kin(_dp(x), psi, pi, _dp(pos), _dp(vel), _dp(J), _dp(Jv))
        return pos, vel

    def impact(x, cur, nxt):
        """The reset map: the feet of nxt \\ cur come to rest."""
        xi = np.zeros(36)
        lib.oracle_wb_impact(_dp(x), _ip(cur), _ip(nxt), psi, pi, 1, _dp(xi), None)
        return xi

    def fall_test(b, r, x, idx):
        if d.fall_height > 0:
            fall_margin[b, r] = min(fall_margin[b, r], abs(x[2] - d.fall_height))
            if x[2] < d.fall_height and first_fall[b, r] < 0:
                first_fall[b, r] = idx
    try:
        for b in range(B):
            for r in range(R):
                if plant is not None:
                    set_links(lib, prow[b, r])
                    gain, damp = prow[b, r, 22:34], prow[b, r, 34:46]
                start = lambda a0, t=bool: np.zeros(4, dtype=t) if a0 is None else np.array(a0[b, r], dtype=t)
                x = x0[b, r].astype(np.float64).copy(); alive = True
                F, E, Sl, NF = start(F0), start(E0), start(Sl0), start(NF0, np.float64)
                mus, muk = (float(MUS[b, r]), float(MUK[b, r])) if fric is not None else (None, None)
                m = 0 if not uni or ter.map_of is None else int(np.asarray(ter.map_of)[b, r])
                lift = -np.inf; pen = -np.inf; vmax = 0.0; dist_sl = 0.0
                ev = events[b][r]
                for s in range(n):
                    p, k, reset = (int(v) for v in smap[:, s])
                    # ---- hsddp_mc.h: kick, fall test, feedback on the noisy state, torque limit
                    if alive and kick is not None and s == d.kick_step:
                        x = x + kick[b, r]
                    X[b, r, s] = x
                    if alive:
                        fall_test(b, r, x, s)
                    z = sim.mc_normals(d.seed, d.first_problem + b, r, s) if noisy else np.zeros(48)      # numbered by the CONTROL step
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
                    if uni:              # a phase change: F <- F n C, E <- E \ C, Sl <- Sl n A
                        Cs = sched[p] > 0
                        F = F & Cs
                        E = E & ~Cs
                        if fric is not None:
                            for f in np.flatnonzero(Sl & ((Cs & ~F) | E)):
                                if k == 0 and s > 0:
                                    ev.append((s, 0, "phase_in_sl", int(f)))
                            Sl = Sl & ((Cs & ~F) | E)

                    def solve(A, ft=None):
                        """One solve from x on the feet A: hsddp_plant.h's torque of the state it starts from, hsddp_friction.h's probe."""
                        xn = np.zeros(36); y = np.zeros(12); wt = np.zeros((4, 2))
                        ue = u if plant is None else np.ascontiguousarray(gain * u - damp * x[24:36])
                        if fric is None:
                            lib.oracle_wb_dynamics(_dp(x), _dp(ue), _ip(A), psi, pi, C.c_double(D[p].BG_alpha), C.c_double(h), _dp(xn), _dp(y))
                        else:
                            lib.fric_ref_dynamics(_dp(x), _dp(ue), _ip(A), _ip(Sl), _dp(np.ascontiguousarray(ft)), psi, pi, C.c_double(D[p].BG_alpha), C.c_double(h),
                                                  _dp(xn), _dp(y), _dp(wt))
                        solves[b, r] += 1
                        return xn, y, wt
                    for j in range(S):   # ---- hsddp_substep.h
                        counted[b, r, s, j] = True
                        tested = ((F & Cs) | (~Cs & ~E if ter.early else False)) if uni else np.zeros(4, dtype=bool)
                        if tested.any():             # ---- hsddp_contact.h rule 1, hsddp_terrain.h: landing
                            pos, vel = foot_kin(x)
                            zg = z_ground + sim.terrain_height(ter, pos[:, :2], m)
                            dz = pos[:, 2] - zg; wz = vel[:, 2]
                            thr = np.where(Cs, 0.0, -ter.w_td)
                            if (F & Cs).any():
                                lift = max(lift, float(dz[F & Cs].max()))
                            T = tested & (dz <= 0.0) & (wz < thr)
                            for f in np.flatnonzero(tested):
                                wv = wz[f] - thr[f]
                                raw_kin[0] = min(raw_kin[0], abs(dz[f])); raw_kin[1] = min(raw_kin[1], abs(wv))
                                mg = min(abs(dz[f]), abs(wv)) if T[f] else max(abs(dz[f]) if dz[f] > 0.0 else 0.0, abs(wv) if wv >= 0.0 else 0.0)
                                kin_margin[b, r] = min(kin_margin[b, r], mg, edge_margin(ter, H, m, pos[f, :2]))
                                ix = np.floor((pos[f, 0] - ter.x0) / ter.cx); iy = np.floor((pos[f, 1] - ter.y0) / ter.cy)
                                raw_ix[0] = min(raw_ix[0], ix); raw_ix[1] = max(raw_ix[1], ix); raw_iy[0] = min(raw_iy[0], iy); raw_iy[1] = max(raw_iy[1], iy)
                                cells.add((m, int(np.clip(iy, 0, H.shape[1] - 1)), int(np.clip(ix, 0, H.shape[2] - 1))))
                            if T.any():
                                pen = max(pen, float((-dz[T]).max()))
                                land_z[b, r] = np.nanmin([land_z[b, r, 0], pos[T, 2].min()]), np.nanmax([land_z[b, r, 1], pos[T, 2].max()])
                                x = impact(x, np.zeros(4), T)
                                F = F & ~T; rows["n_land"][b, r] += int((T & Cs).sum())
                                Te = T & ~Cs
                                if Te.any():
                                    E = E | Te; trows["n_early"][b, r] += int(Te.sum())
                                    if trows["first_early"][b, r] < 0:
                                        trows["first_early"][b, r] = s
                        if fric is not None:
                            fresh = np.zeros(4, dtype=bool); tdir = np.zeros((4, 2))
                            wtk = foot_kin(x)[1][:, :2] if Sl.any() else np.zeros((4, 2))      # the tangential foot velocities at the state every solve of this substep starts from
                        while True:
                            A = (Cs & ~F) | E if uni else sched[p]
                            ft = np.zeros((4, 2)) if fric is not None else None
                            for f in np.flatnonzero(Sl):     # ---- hsddp_friction.h, the solve's own decisions: kinetic direction or re-stick (without friction Sl is empty)
                                if fresh[f]:
                                    ft[f] = muk * NF[f] * tdir[f]
                                    continue
                                sp = float(np.hypot(wtk[f, 0], wtk[f, 1]))
                                stick_margin[b, r] = min(stick_margin[b, r], abs(sp - fric.v_stick))
                                if sp > fric.v_stick:
                                    ft[f] = -muk * NF[f] * wtk[f] / sp
                                    if not ev or ev[-1] != (s, j, "kinetic", int(f)):      # (once per substep: the solve may be repeated)
                                        ev.append((s, j, "kinetic", int(f)))
                                else:
                                    Sl[f] = False
                                    frows["n_restick"][b, r] += 1; ev.append((s, j, "restick", int(f)))
                            xn, y, wt = solve(A, ft)
                            if not uni:
                                break
                            lam = y.reshape(4, 3)
                            lz = lam[:, 2]
                            if A.any():
                                force_margin[b, r] = min(force_margin[b, r], float(np.abs(lz[A] - fz_rel).min()))
                            if A.any() and lz[A].min() < fz_rel:     # ---- hsddp_contact.h rule 2: lift-off, first
                                cand = np.where(A, lz, np.inf)
                                f = int(np.argmin(cand))                 # (the lowest leg index on a tie)
                                if A.sum() > 1:
                                    force_margin[b, r] = min(force_margin[b, r], float(np.sort(cand)[1] - cand[f]))
                                if Sl[f]:
                                    ev.append((s, j, "release_sliding", f)); Sl[f] = False
                                if Cs[f]:
                                    F[f] = True
                                    rows["n_release"][b, r] += 1
                                    if rows["first_release"][b, r] < 0:
                                        rows["first_release"][b, r] = s
                                else:
                                    E[f] = False
                                    trows["n_early_release"][b, r] += 1
                                continue
                            if fric is not None and (A & ~Sl).any():     # ---- hsddp_friction.h: onset
                                stick = A & ~Sl
                                lt = np.hypot(lam[:, 0], lam[:, 1])
                                mf = np.where(stick, mus * lz - lt, np.inf)
                                onset_margin[b, r] = min(onset_margin[b, r], float(np.abs(mf[stick]).min()))
                                if mf.min() < 0.0:
                                    f = int(np.argmin(mf))
                                    if stick.sum() > 1:
                                        which_margin[b, r] = min(which_margin[b, r], float(np.sort(mf)[1] - mf[f]))
                                    Sl[f] = True; fresh[f] = True
                                    NF[f] = max(lz[f], 0.0); tdir[f] = lam[f, :2] / lt[f] if lt[f] > 0.0 else 0.0
                                    frows["n_onset"][b, r] += 1; ev.append((s, j, "onset", f))
                                    if frows["first_slide"][b, r] < 0:
                                        frows["first_slide"][b, r] = s
                                    continue
                            break
                        for f in np.flatnonzero(Sl):                 # end of the substep: a sliding foot's force is (f_t, lambda_z); n_f; the row's running values
                            lam[f, :2] = ft[f]                       # (lam is y, by foot)
                            NF[f] = max(lz[f], 0.0)
                            sp = float(np.hypot(wt[f, 0], wt[f, 1]))
                            dist_sl += sp * h; vmax = max(vmax, sp)
                            if not Cs[f]:
                                ev.append((s, j, "slide_e", int(f)))
                        Y[b, r, s, j] = y
                        if uni:
                            att[b, r, s, j] = A; slide[b, r, s, j] = Sl
                            rows["n_free"][b, r] += int((F & Cs).sum()); trows["n_held"][b, r] += int(E.sum()); frows["n_slide"][b, r] += int(Sl.sum())
                        nsq = float(xn @ xn)
                        if not (nsq <= 1e12):      # the divergence test after EVERY substep: the state the failing step was taken from is kept, nothing further is counted
                            first_bad[b, r] = s; alive = False
                            break
                        x = xn
                    if alive and reset:
                        x = impact(x, sched[p], sched_next[p])
                X[b, r, n] = x
                if alive:
                    fall_test(b, r, x, n)
                Fend[b, r] = F; Eend[b, r] = E; Slend[b, r] = Sl; NFend[b, r] = NF
                rows["free_final"][b, r] = bits(F); rows["max_lift"][b, r] = lift if np.isfinite(lift) else 0.0
                trows["early_final"][b, r] = bits(E); trows["max_pen"][b, r] = pen if np.isfinite(pen) else 0.0
                frows["slide_final"][b, r] = bits(Sl); frows["max_speed"][b, r] = vmax; frows["distance"][b, r] = dist_sl
                if uni:
                    pz_final[b, r] = foot_kin(x)[0][:, 2] if np.isfinite(x).all() else np.nan
    finally:
        if plant is not None:
            set_links(lib, np.array(abi.PLANT_NOMINAL))
    if fric is not None:
        force_margin = np.minimum(force_margin, np.minimum(onset_margin, which_margin))
        kin_margin = np.minimum(kin_margin, stick_margin)
    return dict(X=X, U=U, Y=Y, counted=counted, att=att, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin,
                rows=rows, F=Fend, solves=solves, force_margin=force_margin, kin_margin=kin_margin, raw_kin=tuple(raw_kin),
                trows=trows, E=Eend, raw_ix=tuple(raw_ix), raw_iy=tuple(raw_iy), cells=cells, pz_final=pz_final, land_z=land_z,
                frows=frows, Sl=Slend, NF=NFend, slide=slide, onset_margin=onset_margin, which_margin=which_margin, stick_margin=stick_margin, events=events)


# ---- the plumbing of the host builds (tests/_emu/*.cpp behind numpy arguments)

EMU_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc")]
ORACLE_FLAGS = ["-O3", "-march=native", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-shared", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
                "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]      # those of oracle/Makefile


def build_so(tmpdir, source, name, flags=EMU_FLAGS):
    """tests/_emu/<source> compiled with g++ into tmpdir/<name>: a kernel program's host build (EMU_FLAGS), or the oracle with a probe added (ORACLE_FLAGS)."""
    out = os.path.join(str(tmpdir), name)
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "_emu", source), "-o", out])
    return C.CDLL(out)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def policy_arrays(so, b):
    """Problem b of a solved handle as the host builds take it: nph, horizons, dt, BG_alpha, contact [nph, 4], touchdown [nph, 4] and per phase XBAR, UBAR, K."""
    nph = len(so.phases)
    D = [p["desc"] for p in so.phases]
    hor = np.array([q.horizon for q in D], dtype=np.int32); dt = np.array([q.dt for q in D]); al = np.array([q.BG_alpha for q in D])
    ct = np.array([[q.contact[l] for l in range(4)] for q in D], dtype=np.int32)
    td = np.array([[1 if (q.contact[l] == 0 and q.next_contact[l] == 1) else 0 for l in range(4)] for q in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]      # column-major 12 x 36 per knot
    return nph, hor, dt, al, ct, td, xb, ub, kk


def emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min, keep_traj=True):
    """What every *_emu_run begins with, nph .. Y, for problem b of a solved handle; x0, kick: [R, 36]; dist / kick None: the plain walk, else the
    disturbed one; mu > 0: with records.  Returns (args, out, keep): the argument list, the raw output arrays xf, rows, X, U, extra, g, Y it points to,
    and the policy arrays the caller holds until the call has returned (args holds their addresses only)."""
    nph, hor, dt, al, ct, td, xb, ub, kk = keep = policy_arrays(so, b)
    ptrs = lambda arrs: (C.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n, R = smap.shape[1], x0.shape[0]
    x0 = np.ascontiguousarray(x0); smap = np.ascontiguousarray(smap, dtype=np.int32)
    out = dict(xf=np.zeros((R, 36)), rows=np.zeros((R, 5)), X=np.zeros((R, n + 1, 36)), U=np.zeros((R, n, 12)), extra=np.full((R, 2), np.nan),
               g=np.full((R, 5), np.nan), Y=np.full((R, n, 12), np.nan))
    traj = lambda k: vp(out[k]) if keep_traj else None
    use_mc = dist is not None or kick is not None
    d = dist if dist is not None else pkg.sim.Disturbance()
    sw = np.array([d.sigma_u, d.sigma_q, d.sigma_v, d.u_max, d.fall_height])
    kick = None if kick is None else np.ascontiguousarray(kick)
    args = [nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), C.c_double(PSI_DYN), vp(smap), n, R, vp(x0), vp(out["xf"]), vp(out["rows"]),
            traj("X"), traj("U"), int(S), 1 if use_mc else 0, C.c_ulonglong(d.seed), d.first_problem + b, vp(sw), d.kick_step, vp(kick), vp(out["extra"]),
            C.c_double(mu), C.c_double(fz_min), vp(out["g"]), traj("Y")]
    return args, out, keep


def emu_contact_args(R, fz_rel, z_ground, F, hold, *more):
    """The arguments of the contact rule, fz_rel .. hold, and the raw contact rows c [R, 6] they point to; F and `more`: the hand-over arrays (None or
    float [R, 4], updated in place by the run), checked here."""
    for a in (F,) + more:
        assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (R, 4))
    c = np.full((R, 6), np.nan)
    hold = None if hold is None else np.ascontiguousarray(hold, dtype=np.int32)
    return [C.c_double(fz_rel), C.c_double(z_ground), vp(c), vp(F), vp(hold)], c


def emu_terrain_args(R, ter, map_of, E):
    """The arguments of the terrain, t .. E, and the raw terrain rows tr [R, 6] they point to; ter None: the run has no terrain."""
    t = None if ter is None else ter.to_c()
    H = None if ter is None else ter.grid()
    mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
    tr = np.full((R, 6), np.nan)
    return [None if t is None else C.byref(t), vp(H), vp(mo), vp(tr), vp(E)], tr


def struct_rows(raw, dtype):
    """Raw rows of doubles [..., k] as the structured `dtype` (its pad skipped): the integer fields are whole numbers in doubles, asserted, and cast."""
    out = np.zeros(raw.shape[:-1], dtype=dtype)
    for i, f in enumerate(name for name in dtype.names if name != "pad"):
        assert dtype[f].kind != "i" or np.array_equal(raw[..., i], np.round(raw[..., i])), f
        out[f] = raw[..., i]
    return out
