"""Shared by tests/test_terrain_host.py and tests/test_terrain_gpu.py: the reference of a closed-loop window with TERRAIN HEIGHT MAPS AND EARLY SWING-FOOT
TOUCHDOWN (include/hsddp_terrain.h), the host build of the program (tests/_emu/ter_emu.cpp) behind numpy arguments, and the comparison.

Reference: uni_common.oracle_walk_uni extended by the rules of the header, in numpy on the oracle's existing probes only - oracle_wb_foot_kin for
the landing tests, oracle_wb_dynamics with the contact array set to the attached feet A = (C \\ F) u E, oracle_wb_impact(x, 0, T) for a landing;
sim.terrain_height is the lookup.  The walk is started from given (F, E) and returns, beside what oracle_walk_uni returns, the terrain rows, E at the
end, and what the cases assert their non-vacuity on (the raw cell indices and the cells of the tested feet).

Tolerances: the project's own, uni_common's.  Floats 1e-8 x scale (sim_common / grf_common), the integers, free_final and early_final EXACTLY, but
for a sample whose REFERENCE comes within grf_common.MARGIN_FACTOR x the bound of a decision; at most ONE such sample per case (uni_common.near_samples
asserts it on the reference).  The decisions and their margins: the two kinds of uni_common (force_margin, kin_margin), and folded into kin_margin
(all are metres or metres per second against the trajectory bound 1e-8):
  - a swing foot's landing test (p_z <= z_g and w_z < -w_td): true - the smaller of |p_z - z_g| and |w_z + w_td|; false - the larger over the
    conditions that fail;
  - for a tested foot whose neighbouring cell holds a different height: the distance of p_x / p_y to that cell edge."""
import ctypes as C
import os
import subprocess

import numpy as np

import sim_common as sc
import mc_common as mc
import grf_common as gc
import sub_common as sub
import uni_common as un
from conftest import ROOT

DP = un.DP
IP = un.IP
_dp = un._dp
INTS_T = ("first_early", "n_early", "n_early_release", "n_held", "early_final")


def _edge_margin(ter, H, m, p):
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


def oracle_walk_ter(pkg, oracle_lib, phases, policy, smap, x0, S, fz_rel, z_ground, ter, dist=None, kick=None, F0=None, E0=None):
    """x0: [B, R, 36]; ter: sim.Terrain (map_of None or [B, R]); F0, E0: None or bool [B, R, 4].  Returns the dict of uni_common.oracle_walk_uni (att
    holds the feet of E too) plus trows (TERRAIN_ROW_DTYPE [B, R]), E [B, R, 4] at the end, raw_ix / raw_iy (smallest and largest raw cell index of a
    tested foot), cells (the set of (m, iy, ix) a tested foot read), pz_final [B, R, 4] (foot heights of the final state), land_z [B, R, 2] (lowest and highest p_z of a foot of a landing set T; NaN: none)."""
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

    def foot_kin(x):
        pos = np.zeros((4, 3)); vel = np.zeros((4, 3)); J = np.zeros((4, 3, 18)); Jv = np.zeros((4, 3, 18))
        oracle_lib.oracle_wb_foot_kin(_dp(x), C.c_double(mc.PSI_DYN), C.c_double(np.pi), _dp(pos), _dp(vel), _dp(J), _dp(Jv))
        return pos, vel
    for b in range(B):
        for r in range(R):
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
                u = np.ascontiguousarray(u)
                Cs = contact[p] > 0
                F = F & Cs                                   # rule 4: F <- F n C, E <- E \ C at a phase change
                E = E & ~Cs
                h = D[p].dt / S

                def solve(A):
                    xn = np.zeros(36); y = np.zeros(12)
                    oracle_lib.oracle_wb_dynamics(_dp(x), _dp(u), np.ascontiguousarray(A, dtype=np.int32).ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi),
                                                  C.c_double(D[p].BG_alpha), C.c_double(h), _dp(xn), _dp(y))
                    solves[b, r] += 1
                    return xn, y
                for j in range(S):
                    counted[b, r, s, j] = True
                    tested = (F & Cs) | ((~Cs & ~E) if ter.early else np.zeros(4, dtype=bool))
                    if tested.any():                         # rule 1: landing
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
                            kin_margin[b, r] = min(kin_margin[b, r], mg, _edge_margin(ter, H, m, pos[f, :2]))
                            ix = np.floor((pos[f, 0] - ter.x0) / ter.cx); iy = np.floor((pos[f, 1] - ter.y0) / ter.cy)
                            raw_ix[0] = min(raw_ix[0], ix); raw_ix[1] = max(raw_ix[1], ix); raw_iy[0] = min(raw_iy[0], iy); raw_iy[1] = max(raw_iy[1], iy)
                            cells.add((m, int(np.clip(iy, 0, H.shape[1] - 1)), int(np.clip(ix, 0, H.shape[2] - 1))))
                        if T.any():
                            pen = max(pen, float((-dz[T]).max()))
                            land_z[b, r] = np.nanmin([land_z[b, r, 0], pos[T, 2].min()]), np.nanmax([land_z[b, r, 1], pos[T, 2].max()])
                            xi = np.zeros(36)
                            oracle_lib.oracle_wb_impact(_dp(x), zero4.ctypes.data_as(IP), T.astype(np.int32).ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
                            x = xi; F = F & ~T; rows["n_land"][b, r] += int((T & Cs).sum())
                            Te = T & ~Cs
                            if Te.any():
                                E = E | Te; trows["n_early"][b, r] += int(Te.sum())
                                if trows["first_early"][b, r] < 0:
                                    trows["first_early"][b, r] = s
                    while True:                              # rule 2: lift-off
                        A = (Cs & ~F) | E
                        xn, y = solve(A)
                        lz = y.reshape(4, 3)[:, 2]
                        if A.any():
                            force_margin[b, r] = min(force_margin[b, r], float(np.abs(lz[A] - fz_rel).min()))
                        if not A.any() or not (lz[A].min() < fz_rel):
                            break
                        cand = np.where(A, lz, np.inf)
                        f = int(np.argmin(cand))                 # (the lowest leg index on a tie)
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
                    if not (nsq <= 1e12):      # rule 3: the state the failing step was taken from is kept, nothing further is counted
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
            Fend[b, r] = F; Eend[b, r] = E
            rows["free_final"][b, r] = int(sum(1 << l for l in range(4) if F[l]))
            rows["max_lift"][b, r] = lift if np.isfinite(lift) else 0.0
            trows["early_final"][b, r] = int(sum(1 << l for l in range(4) if E[l]))
            trows["max_pen"][b, r] = pen if np.isfinite(pen) else 0.0
            pz_final[b, r] = foot_kin(x)[0][:, 2] if np.isfinite(x).all() else np.nan
    for a in (X, U, Y, counted, att):
        a.setflags(write=False)
    return dict(X=X, U=U, Y=Y, counted=counted, att=att, first_bad=first_bad, first_fall=first_fall, n_sat=n_sat, sat_margin=sat_margin, fall_margin=fall_margin,
                rows=rows, F=Fend, solves=solves, force_margin=force_margin, kin_margin=kin_margin, raw_kin=tuple(raw_kin),
                trows=trows, E=Eend, raw_ix=tuple(raw_ix), raw_iy=tuple(raw_iy), cells=cells, pz_final=pz_final, land_z=land_z)


def report(tag, ref):
    t, r = ref["trows"], ref["rows"]
    print(f"[ter] {tag}: early touchdowns {int(t['n_early'].sum())} on {int((t['n_early'] > 0).sum())} of {t.size} samples, early releases {int(t['n_early_release'].sum())}, held pairs "
          f"{int(t['n_held'].sum())}, stance releases {int(r['n_release'].sum())}, stance landings {int(r['n_land'].sum())}, max_pen {t['max_pen'].max():.3e}, max_lift {r['max_lift'].max():.3e}, "
          f"raw ix {ref['raw_ix']}, raw iy {ref['raw_iy']}, cells {sorted(ref['cells'])[:8]}, diverged {int((ref['first_bad'] >= 0).sum())}")


def compare_case(tag, pkg, res, ref, xbar, mu=0.0, fz_min=0.0, fz_rel=None):
    """One run with the contact rule and the terrain on against its reference walk: everything uni_common.compare_case holds (the cap of one left-out
    sample is asserted there, on the reference, before anything is compared), then the terrain rows."""
    report(tag, ref)
    near = un.compare_case(tag, pkg, {k: v for k, v in res.items() if k != "terrain"}, ref, xbar, mu, fz_min, fz_rel)
    keep = ~near
    got, want = res["terrain"], ref["trows"]
    for f in INTS_T:
        assert np.array_equal(got[f][keep], want[f][keep]), (tag, f, got[f], want[f])
    sc.close(f"{tag} max_pen", got["max_pen"][keep], want["max_pen"][keep], scale=1.0)
    return near


# ---- the host build of the program

def build_emu(tmpdir):
    out = os.path.join(str(tmpdir), "libhsddp_ter_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "ter_emu.cpp"), "-o", out])
    lib = C.CDLL(out)
    assert [lib.ter_emu_park_doubles(m) for m in (0, 1)] == [45, 47]      # the parked column of the three kernels, doubles per lane: 24 064 B at most
    return lib


def emu_args(pkg, so, b, x0, smap):
    """The leading arguments of ter_emu_run for problem b of a solved handle (kept alive by the caller through the returned list)."""
    nph = len(so.phases)
    D = [p["desc"] for p in so.phases]
    hor = np.array([q.horizon for q in D], dtype=np.int32); dt = np.array([q.dt for q in D]); al = np.array([q.BG_alpha for q in D])
    ct = np.array([[q.contact[l] for l in range(4)] for q in D], dtype=np.int32)
    td = np.array([[1 if (q.contact[l] == 0 and q.next_contact[l] == 1) else 0 for l in range(4)] for q in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]
    return nph, hor, dt, al, ct, td, xb, ub, kk


def emu_run(lib, pkg, so, b, x0, smap, S, fz_rel, z_ground, ter, map_of=None, dist=None, kick=None, mu=0.0, fz_min=0.0, F=None, E=None, hold=None, expect=0):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; map_of: None or int [R]; F, E: None or float [R, 4], updated in place.
    Returns raw arrays (expect != 0: the return code the call must give, and None)."""
    nph, hor, dt, al, ct, td, xb, ub, kk = emu_args(pkg, so, b, x0, smap)
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
    for a in (F, E):
        assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (R, 4))
    H = ter.grid(); t = ter.to_c()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.ter_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), C.c_double(mc.PSI_DYN), vp(smap), n, R, vp(x0), vp(xf), vp(rows),
                         vp(X), vp(U), int(S), 1 if use_mc else 0, C.c_ulonglong(d.seed), d.first_problem + b, vp(sw), d.kick_step, vp(kick), vp(extra),
                         C.c_double(mu), C.c_double(fz_min), vp(g), vp(Y), C.c_double(fz_rel), C.c_double(z_ground), vp(c), vp(F), vp(hold),
                         C.byref(t), vp(H), vp(mo), vp(tr), vp(E))
    assert rc == expect, (rc, expect)
    return None if expect else dict(xf=xf, rows=rows, X=X, U=U, extra=extra, g=g, Y=Y, c=c, t=tr)


def terrain_rows_of(pkg, raw):
    assert np.array_equal(raw[..., :5], np.round(raw[..., :5]))      # the counters are whole numbers in doubles
    out = np.zeros(raw.shape[:-1], dtype=pkg._abi.TERRAIN_ROW_DTYPE)
    for i, f in enumerate(INTS_T):
        out[f] = raw[..., i]
    out["max_pen"] = raw[..., 5]
    return out


def host_run(lib, pkg, so, xs, smap, S, fz_rel, z_ground, ter, d=None, k=None, mu=0.0):
    mo = None if ter.map_of is None else np.asarray(ter.map_of)
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, fz_rel, z_ground, ter, None if mo is None else mo[b], d, None if k is None else k[b], mu) for b in range(xs.shape[0])]
    res = un.emu_result(pkg, outs, d is not None or k is not None, mu > 0)
    res["terrain"] = terrain_rows_of(pkg, np.stack([o["t"] for o in outs]))
    return res


def library_run(pkg, solver, xs, n_steps, S, fz_rel, z_ground, ter, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=(fz_rel, z_ground), terrain=ter)


# ---- the cases of tests/test_terrain_host.py and tests/test_terrain_gpu.py, on the contact tests' fixture (uni_common: trot 4 x 12, B = 4, R = 8 around
# Xbar[0], 48 steps, fz_rel = -10 N, u_max = 8 N m, the "flight" kick at step 44; z_ground = 0), sized on the CPU with the reference alone.  The planned
# stance feet of the fixture stand at z = 0; its swing feet clear the ground by a few centimetres, so a step of +3 cm is met by most of them.
#   flat        H = 0, early = 0, S = 3: the walk of uni_common's flight case, to be compared with the run without the terrain
#   block       one map of two cells of 10 m, the second from x = 0.15 m on 3 cm higher: the front feet (x = +0.19 +- the stride) cross the riser, the
#               hind feet stay on the low cell; early = 1, w_td = 0.05 m/s; S = 1 and 4
#   maps        three one-cell maps - flat, +3 cm, -2 cm - with map_of[b, r] = (b + r) mod 3, under case D's noise switches (k_sim_quad_mc_ter), S = 4
#   edge        3 problems x 3 samples (a partial wave), S = 5, a 4 x 4 grid of 5 cm cells around the origin with a chequered +-5 mm: every foot is
#               outside the grid, on every side, and reads an edge cell
#   divergence  uni_common's contained divergence on the block terrain
#   episode     (tests/test_terrain_gpu.py) the window of episode_phases: the trot without its leading stance phase, so that every tick of 11 steps
#               starts in a swing phase and ends one knot before its touchdown, where the swing feet that met the block are held: with the same policy
#               the reference ends tick 0 with E = {0} or {0, 3} on all four robots and counts 87 .. 88 held pairs in tick 1.  The block is 2.5 cm
#               here: at 3 cm two of the four robots come within 5.4e-6 and 5.7e-6 of a landing test in tick 0 (the cap is one); at 2.5 cm the
#               smallest landing margin of the three ticks is 1.8e-4, the smallest force margin 1.9 N
W_TD = 0.05
CASES = [("block", 1), ("block", 4), ("maps", 4), ("edge", 5), ("divergence", 4)]


def terrain_of(pkg, case, shape):
    T = pkg.sim.Terrain
    if case == "flat":
        return T(H=np.zeros((1, 1, 1)), early=False)
    if case in ("block", "divergence", "episode"):
        return T(H=np.array([[[0.0, 0.025 if case == "episode" else 0.03]]]), x0=-9.85, y0=-5.0, cx=10.0, cy=10.0, early=True, w_td=W_TD)
    if case == "maps":
        mo = (np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 3
        return T(H=np.array([0.0, 0.03, -0.02]).reshape(3, 1, 1), early=True, w_td=W_TD, map_of=mo.astype(np.int32))
    if case == "edge":
        i = np.arange(4)
        return T(H=0.005 * np.where((i[:, None] + i[None, :]) % 2 == 0, 1.0, -1.0)[None], x0=-0.1, y0=-0.1, cx=0.05, cy=0.05, early=True, w_td=W_TD)
    raise KeyError(case)


def episode_phases(pkg):
    return pkg.problems.wb_trot_problem(schedule=((0, 1, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 0, 0, 1)), horizons=(12, 12, 12, 12), last_next=(0, 1, 1, 0))


def case_setup(pkg, case, xs):
    """(x0, Disturbance, kick, fz_rel, z_ground, Terrain) of a case on the fixture's samples xs [4, 8, 36]."""
    if case == "maps":      # case D's switches with the flight kick
        x0, d, k, fz_rel, zg = un.case_setup(pkg, "roll", xs)
        _, df, k, _, _ = un.case_setup(pkg, "flight", xs)
        d = pkg.sim.Disturbance(seed=d.seed, sigma_u=d.sigma_u, sigma_q=d.sigma_q, sigma_v=d.sigma_v, u_max=df.u_max, fall_height=d.fall_height, kick_step=df.kick_step)
    else:
        x0, d, k, fz_rel, zg = un.case_setup(pkg, {"flat": "flight", "block": "flight", "edge": "partial", "divergence": "divergence"}[case], xs)
    return x0, d, k, fz_rel, zg, terrain_of(pkg, case, x0.shape[:2])


def assert_case_is_not_vacuous(case, ref, ter):
    """What the case is for, asserted on the reference alone."""
    t, r = ref["trows"], ref["rows"]
    if case == "block":
        assert (t["n_early"] > 0).sum() > t.size // 2, "early touchdowns on fewer than half of the samples"
        assert (t["n_early_release"] > 0).any() and (r["n_release"] > 0).any() and (r["n_land"] > 0).any()
        assert {(0, 0, 0), (0, 0, 1)} <= ref["cells"], "no tested foot in one of the two cells"
    if case == "maps":
        mo = np.asarray(ter.map_of)
        assert all((mo == m).any() for m in range(3)) and (t["n_early"] > 0).any()
    if case == "edge":
        H = ter.grid()
        assert ref["raw_ix"][0] < 0 and ref["raw_ix"][1] > H.shape[2] - 1 and ref["raw_iy"][0] < 0 and ref["raw_iy"][1] > H.shape[1] - 1
        assert (t["n_early"] > 0).any()
    if case == "divergence":
        assert ref["first_bad"][1, 1] == 5 and (ref["first_bad"].ravel()[:3] == -1).all()


def assert_pit_samples_land_lower(ref, ter):
    """Case 3 on the reference: every landing of a sample of the pit map (-2 cm) happens at or below -2 cm, every sample of the flat map has a landing
    above that, and a pit sample that released a stance foot saw it at least 2 cm above its ground (the planned ground is the plane z = 0).  The lowest
    final foot heights are printed: a sample of the pit that never lands keeps walking on the planned plane, held by its scheduled constraints, so
    they do not separate the maps."""
    mo = np.asarray(ter.map_of)
    live = ref["first_bad"] < 0
    pit, flat = (mo == 2) & live, (mo == 0) & live
    top = ref["land_z"][..., 1]
    landed = np.isfinite(top)
    low = np.nanmin(ref["pz_final"], axis=-1)
    print(f"[ter] maps: highest landing, pit samples {top[pit & landed]}, flat samples {top[flat & landed]}; lowest final foot, pit {low[pit].min():.4f} .. {low[pit].max():.4f}, "
          f"flat {low[flat].min():.4f} .. {low[flat].max():.4f}; max_lift of the pit samples with a release {ref['rows']['max_lift'][pit & (ref['rows']['n_release'] > 0)]}")
    assert (pit & landed).sum() >= 2 and (flat & landed).sum() >= 2
    assert top[pit & landed].max() <= -0.02 < top[flat & landed].min()
    rel = pit & (ref["rows"]["n_release"] > 0)
    assert rel.any() and (ref["rows"]["max_lift"][rel] >= 0.02 - 1e-3).all()
