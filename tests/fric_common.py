"""Shared by tests/test_friction_host.py and tests/test_friction_gpu.py: the reference of a closed-loop window with COULOMB FRICTION
(include/hsddp_friction.h), the host build of the program (tests/_emu/fric_emu.cpp) behind numpy arguments, and the comparison.

Reference: walk_ref.reference_walk with the contact rule and friction, in numpy.  Every solve is fric_ref_dynamics of tests/_emu/fric_ref.cpp - the
whole oracle plus wb_forward restated with a row mask per foot and an added foot force, built into a temporary directory with the oracle's flags -
oracle_wb_foot_kin gives the foot velocities the kinetic direction and the re-stick test read.  The walk is started from
given (F, E, Sl, n_f) and returns, beside what oracle_walk_ter returns, the friction rows, (Sl, n_f) at the end, the sliding set of every substep's last
solve, and the margins of its new decisions.

Tolerances: the project's own, uni_common's.  Floats sim_common.RTOL x scale (trajectories, summaries, max_speed, distance), grf_common.force_bound on
forces; the integers and slide_final EXACTLY, but for a sample whose REFERENCE comes within grf_common.MARGIN_FACTOR x the bound of a decision; at most
ONE such sample per case (uni_common.near_samples asserts it on the reference, before anything is compared).  The new decisions and their margins:
  - onset: |m_f| = |mu_s lambda_z - |lambda_t|| of every sticking attached foot of every solve the onset test reads, against the force bound (folded
    into force_margin);
  - which foot: the gap between the two smallest m_f at an onset (force_margin);
  - re-stick: | |w_t| - v_stick | of every non-fresh sliding foot of every solve, against the trajectory bound (folded into kin_margin).
The kinetic direction divides by |w_t| > v_stick; the cases use v_stick >= 1e-2 m/s, which keeps a 1e-12 velocity error below the force bound."""
import ctypes as C

import numpy as np

import sim_common as sc
import mc_common as mc
import grf_common as gc
import uni_common as un
import ter_common as tc
import walk_ref as wr
from walk_ref import DP, IP

INTS_F = ("first_slide", "n_onset", "n_slide", "n_restick", "slide_final")
INTS_C = ("first_release", "n_release", "n_land", "n_free", "free_final")


def build_ref(pkg, tmpdir):
    """The oracle with fric_ref_dynamics (tests/_emu/fric_ref.cpp), with the flags of oracle/Makefile."""
    lib = pkg._abi.bind(wr.build_so(tmpdir, "fric_ref.cpp", "liboracle_fric_ref.so", wr.ORACLE_FLAGS))
    lib.fric_ref_dynamics.argtypes = [DP, DP, IP, IP, DP, C.c_double, C.c_double, C.c_double, C.c_double, DP, DP, DP]; lib.fric_ref_dynamics.restype = None
    return lib


def oracle_walk_fric(pkg, ref_lib, phases, policy, smap, x0, S, fz_rel, z_ground, ter, fric, dist=None, kick=None, F0=None, E0=None, Sl0=None, NF0=None):
    """x0: [B, R, 36]; ter: sim.Terrain or None (the flat one-cell map without early touchdown); fric: sim.Friction; F0, E0, Sl0: None or bool [B, R, 4];
    NF0: None or float [B, R, 4].  Returns the dict of ter_common.oracle_walk_ter plus frows (FRICTION_ROW_DTYPE [B, R]), Sl and NF [B, R, 4] at the end,
    slide [B, R, n, S, 4] (the sliding set of every substep's last solve), onset_margin / which_margin / stick_margin [B, R] (already folded into
    force_margin and kin_margin), and events: per sample a list of (step, substep, kind, leg), kind in onset / kinetic (the solve applied the kinetic force on the foot's non-fresh branch) / restick / release_sliding / phase_in_sl / slide_e (a foot of E in Sl at a substep's end)."""
    w = wr.reference_walk(pkg, ref_lib, phases, policy, smap, x0, S, contact=(fz_rel, z_ground), ter=ter, fric=fric, dist=dist, kick=kick, F0=F0, E0=E0, Sl0=Sl0, NF0=NF0)
    return wr.pick(w, wr.KEYS_FRIC)


def grf_rows_fric(pkg, ref, mu, fz_min):
    """The force records of a run with friction: min_fz and max_fz over the attached (foot, substep) pairs that count, min_cone, first_slip and n_slip
    over the STICKING ones."""
    Y = ref["Y"]
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    st = ref["att"] & ref["counted"][..., None]
    sk = st & ~ref["slide"]
    fz = F[..., 2]
    cone = mu * fz - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    viol = sk & ((fz < fz_min) | (cone < 0.0))
    out = np.zeros(Y.shape[:-3], dtype=pkg._abi.GRF_ROW_DTYPE)
    out["min_fz"] = np.where(st, fz, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["min_cone"] = np.where(sk, cone, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["max_fz"] = np.where(st, fz, -np.inf).max(axis=(-3, -2, -1), initial=-np.inf)
    step = viol.any(axis=(-2, -1))
    out["first_slip"] = np.where(step.any(axis=-1), step.argmax(axis=-1), -1)
    out["n_slip"] = viol.sum(axis=(-3, -2, -1))
    rec_margin = np.minimum(np.where(sk, np.abs(cone), np.inf).min(axis=(-3, -2, -1), initial=np.inf), np.where(sk, np.abs(fz - fz_min), np.inf).min(axis=(-3, -2, -1), initial=np.inf))
    return out, rec_margin


def report(tag, ref):
    f = ref["frows"]
    kinds = [k for per_b in ref["events"] for per_r in per_b for (_, _, k, _) in per_r]
    print(f"[fric] {tag}: onsets {int(f['n_onset'].sum())} on {int((f['n_onset'] > 0).sum())} of {f.size} samples, sliding pairs {int(f['n_slide'].sum())}, re-sticks {int(f['n_restick'].sum())}, "
          f"sliding feet released {kinds.count('release_sliding')}, in Sl at a phase change {kinds.count('phase_in_sl')}, two at once {int((ref['slide'].sum(axis=-1) >= 2).sum())} substeps, "
          f"max_speed {f['max_speed'].max():.3e}, distance {f['distance'].max():.3e}; smallest onset margin {ref['onset_margin'].min():.3e} N, which-foot {ref['which_margin'].min():.3e} N, "
          f"re-stick {ref['stick_margin'].min():.3e} m/s; releases {int(ref['rows']['n_release'].sum())}, landings {int(ref['rows']['n_land'].sum())}, diverged {int((ref['first_bad'] >= 0).sum())}")


def compare_case(tag, pkg, res, ref, xbar, mu=0.0, fz_min=0.0, fz_rel=None):
    """One run with the contact rule and friction on against its reference walk: the cap of one left-out sample on the reference first (with the
    records' own margins over the sticking feet), then everything uni_common.compare_case holds on trajectories, summaries and contact rows, the force
    records by this header's rule, the terrain rows if the run has them, and the friction rows."""
    report(tag, ref)
    want_g, rec_margin = grf_rows_fric(pkg, ref, mu, fz_min) if "grf" in res else (None, None)
    near = un.near_samples(tag, ref, rec_margin)
    un.compare_case(tag, pkg, {k: v for k, v in res.items() if k not in ("terrain", "friction", "grf", "Y")}, ref, xbar, 0.0, 0.0, None)
    keep = ~near
    if "grf" in res:
        bound = gc.force_bound(ref["Y"]); scale = bound / sc.RTOL
        if res.get("Y") is not None:
            cnt = ref["counted"][keep][..., 0]      # the steps a sample was alive at: behind first_bad the reference records nothing
            sc.close(tag + " Y", res["Y"][keep][cnt], ref["Y"][keep][..., 0, :][cnt], scale=scale)
            free = ~np.repeat(ref["att"][keep][..., 0, :], 3, axis=-1)
            assert (res["Y"][keep][cnt][free[cnt]] == 0.0).all(), f"{tag}: the force entry of a foot that is not attached is not exactly 0"
        for f in ("min_fz", "min_cone", "max_fz"):
            a, w = res["grf"][f][keep], want_g[f][keep]
            assert np.array_equal(np.isfinite(a), np.isfinite(w)) and np.array_equal(a[~np.isfinite(w)], w[~np.isfinite(w)]), (tag, f)
            sc.close(f"{tag} {f}", a[np.isfinite(w)], w[np.isfinite(w)], scale=scale)
        assert np.array_equal(res["grf"]["first_slip"][keep], want_g["first_slip"][keep]), (tag, res["grf"]["first_slip"], want_g["first_slip"])
        assert np.array_equal(res["grf"]["n_slip"][keep], want_g["n_slip"][keep]), (tag, res["grf"]["n_slip"], want_g["n_slip"])
        if fz_rel is not None:
            fin = np.isfinite(res["grf"]["min_fz"])
            assert (res["grf"]["min_fz"][fin] >= fz_rel - bound).all(), tag
    if "terrain" in res:
        for f in tc.INTS_T:
            assert np.array_equal(res["terrain"][f][keep], ref["trows"][f][keep]), (tag, f, res["terrain"][f], ref["trows"][f])
        sc.close(f"{tag} max_pen", res["terrain"]["max_pen"][keep], ref["trows"]["max_pen"][keep], scale=1.0)
    got, want = res["friction"], ref["frows"]
    for f in INTS_F:
        assert np.array_equal(got[f][keep], want[f][keep]), (tag, f, got[f], want[f])
    live = keep & (ref["first_bad"] < 0) if (ref["first_bad"] >= 0).any() else keep
    xs = max(1.0, float(np.abs(ref["X"][live]).max()))      # the foot velocities are the state's velocities through Jacobians of order one
    sc.close(f"{tag} max_speed", got["max_speed"][keep], want["max_speed"][keep], scale=xs)
    sc.close(f"{tag} distance", got["distance"][keep], want["distance"][keep], scale=xs)
    return near


# ---- the host build of the program

def build_emu(tmpdir):
    lib = wr.build_so(tmpdir, "fric_emu.cpp", "libhsddp_fric_emu.so")
    assert [lib.fric_emu_park_doubles(m) for m in (0, 1)] == [61, 63]      # the parked column of the three kernels, doubles per lane: 32 256 B at most
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, fz_rel, z_ground, ter, fric, mu_of=None, map_of=None, dist=None, kick=None, mu=0.0, fz_min=0.0, F=None, E=None, Sl=None, NF=None, hold=None, expect=0):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; ter: sim.Terrain or None; mu_of, map_of: None or int [R]; F, E, Sl, NF: None or
    float [R, 4], updated in place.  Returns raw arrays (expect != 0: the return code the call must give, and None)."""
    R = x0.shape[0]
    args, out, keep = wr.emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min)
    ctail, out["c"] = wr.emu_contact_args(R, fz_rel, z_ground, F, hold, E, Sl, NF)
    ttail, out["t"] = wr.emu_terrain_args(R, ter, map_of, E)
    fo = None if mu_of is None else np.ascontiguousarray(mu_of, dtype=np.int32)
    mu_t = fric.table(); fp = pkg._abi.FrictionParams(fric.v_stick, mu_t.shape[0], 0)
    out["f"] = np.full((R, 7), np.nan)
    rc = lib.fric_emu_run(*args, *ctail, *ttail, C.byref(fp), wr.vp(mu_t), wr.vp(fo), wr.vp(out["f"]), wr.vp(Sl), wr.vp(NF))
    assert rc == expect, (rc, expect)
    return None if expect else out


def friction_rows_of(pkg, raw):
    return wr.struct_rows(raw, pkg._abi.FRICTION_ROW_DTYPE)


def host_run(lib, pkg, so, xs, smap, S, fz_rel, z_ground, ter, fric, d=None, k=None, mu=0.0):
    mo = None if ter is None or ter.map_of is None else np.asarray(ter.map_of)
    fo = None if fric.mu_of is None else np.asarray(fric.mu_of)
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, fz_rel, z_ground, ter, fric, None if fo is None else fo[b], None if mo is None else mo[b], d, None if k is None else k[b], mu)
            for b in range(xs.shape[0])]
    res = un.emu_result(pkg, outs, d is not None or k is not None, mu > 0)
    if ter is not None:
        res["terrain"] = tc.terrain_rows_of(pkg, np.stack([o["t"] for o in outs]))
    res["friction"] = friction_rows_of(pkg, np.stack([o["f"] for o in outs]))
    return res


def library_run(pkg, solver, xs, n_steps, S, fz_rel, z_ground, ter, fric, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=(fz_rel, z_ground), terrain=ter, friction=fric)


# ---- the cases of tests/test_friction_host.py and tests/test_friction_gpu.py, on the contact tests' fixture (uni_common: trot 4 x 12, B = 4, R = 8 around
# Xbar[0], 48 steps, fz_rel = -10 N, u_max = 8 N m; z_ground = 0), sized on the CPU with the reference alone (SIZING below).
V_STICK = 0.02
MU_BIG = 1e9


def friction_of(pkg, case, shape):
    """The table of a case: row 0 never slides (mu_s = 1e9), row 1 moderate, row 2 low; sample 0 of every problem is the control sample on row 0."""
    Fr = pkg.sim.Friction
    if case == "none":
        return Fr(mu=[[MU_BIG, MU_BIG]], v_stick=V_STICK)
    B, R = shape
    if case == "block":      # (its own subset of the fixture: every sample but the first of a problem may slide)
        mo = 1 + (np.arange(B)[:, None] + np.arange(R)[None, :]) % 2
        mo[:, 0] = 0
    else:
        mo = np.zeros((B, R), dtype=np.int64)
        for (b, r), row in (SLIDERS_NOISE if case == "noise" else SLIDERS).items():
            mo[b, r] = row
    return Fr(mu=[[MU_BIG, MU_BIG], [MU_MOD, MU_MOD_K], [MU_LOW, MU_LOW_K]], mu_of=mo.astype(np.int32), v_stick=V_STICK)


# SIZING, with the reference alone (tests/test_friction_host.py::test_amplification_through_the_friction_windows prints the amplification of a 1e-12 change
# of x0 through every case).  What shaped the cases: on this fixture the planned trot itself leaves the cone - at mu = 0.5 / 0.25, 26 of the 32 samples slide
# without any push, 205 .. 220 onsets, forces up to 1e6 N and ten divergences at S = 1 (the explicit friction force is first order in dt / S), and two to
# thirty samples of the reference within the margin of a decision.  So the table is mild - row 1 (0.9, 0.8), row 2 (0.7, 0.6) - which leaves 12 of 32 samples
# sliding, 40 onsets at S = 1, forces below 160 N at S = 4 (force bound 7.9e-7 N), and NO sample of the reference within the margins at S = 1 and S = 4
# (smallest onset margin 7.9e-3 N against the needed 1.6e-3, smallest re-stick margin 8e-3 m/s against 1e-5); (mu 0.9 / 0.6 loses the re-stick at S = 1,
# 0.8 / 0.7 the released sliding foot at S = 4).  But a sliding sample of this closed loop amplifies a 1e-12 change of x0 by up to 2.5e8 x at S = 1 and 5e6 x at
# S = 4 (sample (1, 2) even diverges at S = 1), against the 100 x |X|max the windows' tolerance allows (tests/test_contact_host.py's criterion).  So only the
# samples of SLIDERS are on rows 1 and 2 - those that amplify at most 6e3 x at S = 1 (|X|max 212) and 3e2 x at S = 4 (|X|max 9) - and between them they show
# every event the push case is for, but a released sliding foot at S = 4: the one sample that has one there, (2, 2) on row 1, amplifies 1.6e6 x.  Every other
# sample is on row 0, mu_s = 1e9.  Such a sample still slides when a foot PULLS (lambda_z < 0 is outside the cone at any mu): (2, 2), which pulls with 6 N at
# its first steps, has an onset at step 0 with n_f = 0, slides freely and fails the divergence test at step 2 .. 3 with forces of 3e9 N, a force bound of
# 28 N for the whole case.  The push and noise cases replace it by a copy of sample (2, 5).
# The push is lateral (base velocity y, coordinate 19, 0 .. 1 m/s over the eight samples) at step 38, a trot
# stance step, under the 8 N m torque limit of the contact tests' kicked cases; its size (1.0 or 1.5) and step (38 or 40) do not move these figures.
#   none        mu_s = 1e9 on the contact tests' flight case with fz_rel = 0: at ANY mu a foot with lambda_z < 0 is outside the cone, so with the fixture's
#               fz_rel = -10 N eleven onsets happen at mu_s = 1e9 (feet that pull with less than 10 N); with fz_rel = 0 such a foot is released first
#   push        S = 1 and 4, the three-row table, sample 0 of every problem on row 0 (it never slides)
#   partial     3 problems x 3 samples, S = 5
#   noise       case D's noise on top (k_sim_quad_mc_fric), S = 4
#   block       ter_common's block with early touchdown, problem 0, samples 4 .. 7, S = 2: feet of E slide (all 32 samples at S = 4 put 14 of them within
#               the margins - 172 onsets - and one diverges with forces of 1e8 N; this subset has none within them, |X| below 10, amplification 40 x)
#   divergence  uni_common's contained divergence; the diverging sample alone on a row (0.2, 0.1), so that it slides when it fails the test in substep 1
MU_MOD, MU_MOD_K = 0.9, 0.8
MU_LOW, MU_LOW_K = 0.7, 0.6
PUSH, PUSH_STEP = 1.0, 38
NONE_FZ_REL = 0.0
SLIDERS = {(0, 3): 2, (2, 1): 2, (1, 7): 1, (3, 4): 2}      # the samples that may slide and their rows of the table; every other sample is a control sample on row 0
SLIDERS_NOISE = {(2, 1): 2, (1, 7): 1}                     # ... under noise, where (0, 3) and (3, 4) amplify a 1e-12 change 2e4 x and 3e3 x
DIV_MU = 0.2
BLOCK_FZ_REL = un.FZ_REL
BLOCK_SEL = (0, 1, 4, 8)
# the three-tick episode of tests/test_friction_gpu.py (sized on the device, where its policy comes from): the friction row of every robot and the lateral
# push (m/s, base velocity y) at step 0 of every tick.  At (0.3, 0.25) without a push the planned gait slides by itself: three robots end tick 0 and two end
# tick 1 with a foot sliding, robot 0 slides through all 44 substeps of ticks 1 and 2 without an onset in them, no robot comes within the margins (smallest
# force margin 5e-2 N against the needed 7e-4), none diverges.  Rows (0.5, 0.4) and (0.7, 0.6) without a push carry nothing into a later tick.
EPISODE_MU, EPISODE_PUSH = (0.3, 0.25), 0.0
CASES = [("push", 1), ("push", 4), ("partial", 5), ("noise", 4), ("block", 2), ("divergence", 4)]


def case_setup(pkg, case, xs):
    """(x0, Disturbance, kick, fz_rel, z_ground, Terrain or None, Friction) of a case on the fixture's samples xs [4, 8, 36]."""
    Dist = pkg.sim.Disturbance
    ramp = np.linspace(0.0, 1.0, 8)[None, :]
    if case == "none":      # (fz_rel = 0: a foot that pulls is released before the onset test sees it - at any mu a foot with lambda_z < 0 is outside the cone)
        x0, d, k, fz_rel, zg = un.case_setup(pkg, "flight", xs)
        return x0, d, k, NONE_FZ_REL, zg, None, friction_of(pkg, case, x0.shape[:2])
    if case == "block":
        b0, b1, r0, r1 = BLOCK_SEL
        xs = np.ascontiguousarray(xs[b0:b1, r0:r1]); ramp = ramp[:, r0:r1]
    if case in ("push", "noise"):      # sample (2, 2) pulls at its first steps, slides freely at any mu and diverges with forces of 1e9 N, which would set the
        xs = xs.copy(); xs[2, 2] = xs[2, 5]      # force bound of the whole case: its place is taken by a copy of sample (2, 5)
    if case in ("push", "block"):
        k = np.zeros(xs.shape); k[..., 19] = PUSH * ramp
        ter = tc.terrain_of(pkg, "block", xs.shape[:2]) if case == "block" else None
        return xs, Dist(seed=mc.SEED, u_max=8.0, kick_step=PUSH_STEP), k, BLOCK_FZ_REL if case == "block" else un.FZ_REL, 0.0, ter, friction_of(pkg, case, xs.shape[:2])
    if case == "noise":
        Dn = mc.cases(pkg, xs.shape[:2])["D"][0]
        k = np.zeros(xs.shape); k[..., 19] = PUSH * ramp
        d = Dist(seed=mc.SEED, sigma_u=Dn.sigma_u, sigma_q=Dn.sigma_q, sigma_v=Dn.sigma_v, u_max=Dn.u_max, fall_height=Dn.fall_height, kick_step=PUSH_STEP)
        return xs, d, k, un.FZ_REL, 0.0, None, friction_of(pkg, case, xs.shape[:2])
    if case == "partial":
        x0 = np.ascontiguousarray(xs[:3, 5:8])
        k = np.zeros(x0.shape); k[..., 19] = PUSH * ramp[:, 5:8]
        fr = friction_of(pkg, case, (4, 8))
        fr = pkg.sim.Friction(mu=fr.mu, mu_of=np.ascontiguousarray(fr.mu_of[:3, 5:8]), v_stick=fr.v_stick)
        return x0, Dist(seed=mc.SEED, u_max=8.0, kick_step=PUSH_STEP), k, un.FZ_REL, 0.0, None, fr
    if case == "divergence":
        x0 = np.ascontiguousarray(xs[:2, :2])
        k = np.zeros(x0.shape); k[1, 1, 23] = 1e4
        mo = np.zeros(x0.shape[:2], dtype=np.int32); mo[1, 1] = 1
        fr = pkg.sim.Friction(mu=[[MU_BIG, MU_BIG], [DIV_MU, DIV_MU / 2]], mu_of=mo, v_stick=V_STICK)
        return x0, Dist(seed=mc.SEED, kick_step=5), k, un.FZ_REL, 0.0, None, fr
    raise KeyError(case)


def assert_case_is_not_vacuous(case, ref, S=None):
    """What the case is for, asserted on the reference alone.  The push case asks for the issue's list - an onset, a substep with two feet sliding, ONE foot
    on its non-fresh (kinetic) branch in consecutive substeps, a re-stick, a foot in Sl at a phase change, a control sample per problem - at S = 1 and at
    S = 4, and for a sliding foot that is then released at S = 1 ONLY: the S = 4 push case is weaker than the issue's list by that one event (SIZING: the one
    sample that has it there amplifies 1.6e6 x), and only the four samples of SLIDERS may slide in it."""
    f = ref["frows"]
    kinds = lambda b, r: [k for (_, _, k, _) in ref["events"][b][r]]
    every = [k for b in range(f.shape[0]) for r in range(f.shape[1]) for k in kinds(b, r)]
    if case in ("push", "partial", "noise", "block"):
        assert f["n_onset"].sum() > 0, "no onset"
    if case == "push":
        sl = ref["slide"]
        assert (sl.sum(axis=-1) >= 2).any(), "no substep with two feet sliding at once"
        nS = sl.shape[3]
        kin = {}      # (problem, sample, leg) -> the global substeps in which the solve took the foot's kinetic branch
        for b in range(f.shape[0]):
            for r in range(f.shape[1]):
                for (s_, j_, k_, l_) in ref["events"][b][r]:
                    if k_ == "kinetic":
                        kin.setdefault((b, r, l_), set()).add(s_ * nS + j_)
        runs = any(g + 1 in v and g + 2 in v for v in kin.values() for g in v)
        assert runs and f["max_speed"].max() > V_STICK, "no foot stays on its kinetic branch across three consecutive substeps"
        assert "restick" in every, "no re-stick"
        assert S != 1 or "release_sliding" in every, "no sliding foot is released"      # (at S = 4 the one sample that does amplifies 1e6 x: SIZING)
        assert "phase_in_sl" in every, "no foot is in Sl at a phase change"
        ctl = np.ones(f.shape, dtype=bool)
        for (b, r) in SLIDERS:
            ctl[b, r] = False
        assert (ctl & (f["n_onset"] == 0)).any(axis=1).all(), "a problem without a control sample that never slides"
    if case == "block":
        assert "slide_e" in every, "no foot of E slides"
    if case == "divergence":
        assert ref["first_bad"][1, 1] == 5 and (ref["first_bad"].ravel()[:3] == -1).all()
        assert ref["slide"][1, 1, 5].any() or f["n_slide"][1, 1] > 0, "the diverging sample does not slide"
