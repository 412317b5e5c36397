"""Sub-stepped integration (include/hsddp_substep.h; kernels k_sim_quad_sub, k_sim_quad_mc_sub, k_sim_quad_mc0_sub, k_sim_quad_grf_sub,
k_sim_quad_mc_grf_sub, k_sim_quad_mc0_grf_sub of cafe-mpc_amd/csrc/wb_sim.hpp) on the device: parity with the reference walk of
tests/sub_common.py, a partial wave, S = 1 and toggling, the prefix property, contained divergence, episodes, refusals, allocation and the
handle left as it was."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import sim_common as sc
import mc_common as mc
import grf_common as gc
import sub_common as sub

pytestmark = pytest.mark.gpu

EINVAL = -1
MU = 0.6
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
Dist = pkg.sim.Disturbance
ep = pkg.episode


@pytest.fixture(scope="module")
def trot12(oracle_lib, hip_lib):
    """trot12 of tests/test_sim_gpu.py on the device: trot 4 x 12, B = 4 (wb_ensemble_x0(4, 20241222)), 3 AL x 4 DDP, R = 8 samples (sigma 0.02 /
    0.2, seed 20241222) around Xbar[0].  The reference walks use the DEVICE handle's policy rows and are computed once per (case, S, n)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    sg = pkg.MultiPhaseDDP(phases, batch=4)
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); sg.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(sg.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    pol = mc.policy_of(sg)
    cache = {}

    def ref(case, S, n=48):
        if (case, S, n) not in cache:
            d, k = mc.cases(pkg, xs.shape[:2])[case] if case in "ABCD" else (None, None)
            cache[(case, S, n)] = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, sc.step_map(phases, n), xs, S, d, k)
        return cache[(case, S, n)]
    yield phases, sg, xs, pol, ref
    sg.close()


def run_case(sg, xs, n, case, S, records=False, keep_traj=True):
    d, k = mc.cases(pkg, xs.shape[:2])[case] if case in "ABCD" else (None, None)
    return sg.simulate(xs, n, keep_traj=keep_traj, dist=d, kick=k, grf=(MU, 0.0) if records else None, substeps=S)


def same_bits(a, b, but=()):
    assert set(a) == set(b)
    for f in a:
        if f not in but:
            assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("case,S", [("plain", 3), ("plain", 4), ("A", 3), ("C", 4), ("D", 4)])
def test_substep_parity_trot_window(trot12, case, S):
    """48 steps (a lift-off and two reset maps): plain (k_sim_quad_sub) at S = 3 and 4, case A (k_sim_quad_mc_sub) at S = 3, case C
    (k_sim_quad_mc0_sub) and case D at S = 4, against the reference walk with the device's own policy.  The lean run gives the same row bytes."""
    phases, sg, xs, pol, ref = trot12
    smap = sc.step_map(phases, 48)
    r = ref(case, S)
    assert (r["first_bad"] == -1).all()
    res = run_case(sg, xs, 48, case, S)
    assert res["X"].shape == (4, 8, 49, 36) and res["U"].shape == (4, 8, 48, 12)
    sub.compare_case(f"gpu {case} S={S}", pkg, res, r, mc.xbar_window(pol, smap))
    lean = run_case(sg, xs, 48, case, S, keep_traj=False)
    assert lean["rows"].tobytes() == res["rows"].tobytes() and np.array_equal(lean["x_final"], res["x_final"])
    one = run_case(sg, xs, 48, case, 1)
    gap = float(np.abs(one["X"] - res["X"]).max())
    print(f"[sub] gpu {case}: largest |X(S={S}) - X(S=1)| = {gap:.3f}, |U| {np.abs(one['U'] - res['U']).max():.3f}, final {np.abs(one['x_final'] - res['x_final']).max():.3f}")
    assert gap > 1e-3


def test_substep_parity_with_records(trot12):
    """Records at S = 4, mu = 0.6 (k_sim_quad_grf_sub): Y is the force of substep 0, a swing leg's entries exactly 0; the three floats over every
    substep; first_slip and n_slip EQUAL to the reference's under the asserted margins (min |cone| 4.0e-3 N against 6.6e-4 N needed)."""
    phases, sg, xs, pol, ref = trot12
    smap = sc.step_map(phases, 48)
    contact = gc.contact_of(phases, smap)
    res = run_case(sg, xs, 48, "plain", 4, records=True)
    assert res["Y"].shape == (4, 8, 48, 12) and res["grf"].shape == (4, 8)
    sub.compare_case("gpu records S=4", pkg, res, ref("plain", 4), mc.xbar_window(pol, smap), contact, MU, 0.0)
    one = run_case(sg, xs, 48, "plain", 1, records=True)
    print(f"[sub] gpu records: n_slip S=4 {int(res['grf']['n_slip'].sum())} (/ 4 = {res['grf']['n_slip'].sum() / 4:.1f}), S=1 {int(one['grf']['n_slip'].sum())}; "
          f"slipping samples {int((res['grf']['first_slip'] >= 0).sum())} / {int((one['grf']['first_slip'] >= 0).sum())}")
    lean = run_case(sg, xs, 48, "plain", 4, records=True, keep_traj=False)
    assert lean["grf"].tobytes() == res["grf"].tobytes()


def test_substep_partial_wave(oracle_lib, hip_lib):
    """B = 3, R = 3 (nine of the sixteen quads of one wave, quads of three problems in it), trot 4 x 6, 24 steps, S = 5: plain and with records
    (margins of the reference measured on the CPU: min |cone| 0.15 N, min |fz| 2.4 N against 4.7e-4 N needed - asserted)."""
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=3); s.set_initial_condition(pkg.problems.wb_ensemble_x0(3, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    smap = sc.step_map(phases, 24)
    pol = mc.policy_of(s)
    ref = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs, 5)
    plain = s.simulate(xs, 24, keep_traj=True, substeps=5)
    sub.compare_case("3 x 3 S=5", pkg, plain, ref, mc.xbar_window(pol, smap))
    rec = s.simulate(xs, 24, keep_traj=True, grf=(MU, 0.0), substeps=5)
    sub.compare_case("3 x 3 S=5 records", pkg, rec, ref, mc.xbar_window(pol, smap), gc.contact_of(phases, smap), MU, 0.0)
    same_bits(plain, {k: v for k, v in rec.items() if k not in ("grf", "Y")})      # the records change nothing else
    assert len({rec["Y"][b, r].tobytes() for b in range(3) for r in range(3)}) == 9
    s.close()


def collect(sim, disturbed):
    rows, xf = sim.rows(); X, U = sim.traj()
    out = dict(rows=rows, x_final=xf, X=X, U=U)
    if disturbed:
        out["extra"] = sim.extra()
    return out


def test_one_substep_and_toggling(trot12):
    """One object: run, set(1), run - identical bits (the same kernels); set(4), run, set(1), run - identical to the first.  With the records on,
    everything but the record rows is bit-identical to the records off at S = 4, for the plain run (k_sim_quad_grf_sub against k_sim_quad_sub),
    case C (torque limit, fall height and a push, no noise: k_sim_quad_mc0_grf_sub against k_sim_quad_mc0_sub, which the parity test holds to the
    reference, first_fall and n_sat included) and case D (k_sim_quad_mc_grf_sub against k_sim_quad_mc_sub)."""
    phases, sg, xs, pol, ref = trot12
    for case in ("plain", "C", "D"):
        d, k = mc.cases(pkg, xs.shape[:2])[case] if case != "plain" else (None, None)
        sim = pkg.Simulation(sg, 8, 48, keep_traj=True)
        assert sim.substeps == 1
        sim.run(xs, dist=d, kick=k); first = collect(sim, d is not None)
        sim.set_substeps(1); assert sim.substeps == 1
        sim.run(xs, dist=d, kick=k); same_bits(collect(sim, d is not None), first)
        sim.set_substeps(4); assert sim.substeps == 4
        sim.run(xs, dist=d, kick=k); four = collect(sim, d is not None)
        assert not np.array_equal(four["X"], first["X"])
        sim.set_grf(MU)
        sim.run(xs, dist=d, kick=k); on = collect(sim, d is not None); same_bits(on, four)
        g, Y = sim.grf()
        assert (g["max_fz"] > 1.0).all() and np.abs(Y).max() > 1.0
        if case == "C":      # (and the extras that are compared are not empty ones)
            assert (on["extra"]["n_sat"] > 0).all() and (on["extra"]["first_fall"] >= 0).any()
        sim.set_substeps(1)
        sim.run(xs, dist=d, kick=k); same_bits(collect(sim, d is not None), first)      # records on, one substep: the kernels with records
        sim.set_grf(0.0)
        sim.run(xs, dist=d, kick=k); same_bits(collect(sim, d is not None), first)
        sim.close()


def test_substep_prefix_property(trot12):
    """Case D at S = 4: steps 0 .. 23 of the 48-step run are the 24-step run (the noise is numbered by the control step)."""
    phases, sg, xs, pol, ref = trot12
    long = run_case(sg, xs, 48, "D", 4)
    short = run_case(sg, xs, 24, "D", 4)
    assert np.array_equal(long["X"][:, :, :24], short["X"][:, :, :24]) and np.array_equal(long["U"][:, :, :24], short["U"])
    assert np.array_equal(long["X"][:, :, 24, :18], short["X"][:, :, 24, :18])      # (entry 24 of the long run lies behind a reset map: positions stay)


def test_substep_divergence_is_contained(trot12, oracle_lib):
    """Sample (2, 5) with a base velocity of 1e7 fails the divergence test in substep 0 of step 0 and keeps its initial state; sample (0, 1) with
    5e5 passes substep 0 and fails in substep 1 (the reference on the CPU), so the state it keeps is NOT the initial one.  first_bad equals the
    reference's, the kept states agree within RTOL x their own scale (host program against reference: 8.7e-13 relative), and every other
    sample is bit-identical to the run without them, records included."""
    phases, sg, xs, pol, ref = trot12
    clean = run_case(sg, xs, 48, "plain", 4, records=True)
    x = xs.copy(); x[2, 5, 18] = 1e7; x[0, 1, 18] = 5e5
    r = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, sc.step_map(phases, 48), x, 4)
    assert r["first_bad"][2, 5] == 0 and r["first_bad"][0, 1] == 0 and (r["first_bad"] >= 0).sum() == 2
    assert r["counted"][2, 5].sum() == 1 and r["counted"][0, 1].sum() == 2      # the failing substep is the last one that counts
    res = sg.simulate(x, 48, keep_traj=True, grf=(MU, 0.0), substeps=4)
    assert np.array_equal(res["rows"]["first_bad"], r["first_bad"]) and (clean["rows"]["first_bad"] == -1).all()
    assert np.array_equal(res["x_final"][2, 5], x[2, 5])
    assert not np.array_equal(r["X"][0, 1, -1], x[0, 1])
    sc.close("kept state of (0, 1)", res["x_final"][0, 1], r["X"][0, 1, -1])
    assert np.array_equal(res["X"][0, 1, 1:], np.broadcast_to(res["x_final"][0, 1], (48, 36)))      # the trajectory repeats the kept state
    keep = np.ones((4, 8), dtype=bool); keep[2, 5] = False; keep[0, 1] = False
    for f in ("x_final", "X", "U", "Y"):
        assert np.array_equal(res[f][keep], clean[f][keep]), f
    assert res["rows"][keep].tobytes() == clean["rows"][keep].tobytes() and res["grf"][keep].tobytes() == clean["grf"][keep].tobytes()


def test_one_tick_episode_is_the_substepped_run(trot12):
    """One sample per problem, 12 steps, S = 4 on the episode's simulation object: rows, state and log bit for bit those of hsddp_sim_run /
    hsddp_mc_run with S = 4 (case D with its push at step 10, and the plain run)."""
    phases, sg, xs, pol, ref = trot12
    x1 = np.ascontiguousarray(xs[:, 1])
    dD, kD = mc.cases(pkg, (4,))["D"]
    for dist, k in ((dD, kD), (None, None)):
        sim = pkg.Simulation(sg, 1, 12, keep_traj=True); sim.set_substeps(4); sim.set_grf(MU)
        sim.run(np.ascontiguousarray(x1[:, None]), dist=dist, kick=None if k is None else np.ascontiguousarray(k[:, None]))
        srows, xf = sim.rows(); X, U = sim.traj(); g, Y = sim.grf(); sim.close()
        one = sg.simulate(np.ascontiguousarray(x1[:, None]), 12, keep_traj=True, dist=dist, kick=None if k is None else np.ascontiguousarray(k[:, None]))
        assert not np.array_equal(one["X"], X)      # (and S = 4 is not S = 1)
        e = sg.episode(12, 1, keep_log=True); e.set_substeps(4); e.set_grf(MU); assert e.substeps == 4
        e.reset(x1); e.advance(dist, k)
        rows, x_now = e.rows(); eX, eU, eY = e.log()
        for f in ("dev_q", "dev_v", "min_height", "max_torque"):
            assert np.array_equal(rows[f], srows[f][:, 0]), f
        for f in ("min_fz", "min_cone", "max_fz", "n_slip", "first_slip"):
            assert np.array_equal(rows[f], g[f][:, 0]), f
        assert np.array_equal(x_now, xf[:, 0]) and np.array_equal(eX, X[:, 0]) and np.array_equal(eU, U[:, 0]) and np.array_equal(eY, Y[:, 0])
        e.close()
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222))


def test_three_tick_episode_is_the_manual_loop(hip_lib):
    """Trot 4 x 12, B = 4, n_exec = 12, three ticks of case D (noise, torque limit, fall height, a push at step 10 of every tick) with the
    records on and S = 4, hsddp_reconfigure between the ticks (the same window again: the episode rebinds its step map, the setting stays).  The
    manual path on a second handle: per tick a fresh Simulation with hsddp_substep_set and hsddp_grf_set, run with tick_seed, read back,
    fold_rows in numpy, set_initial_condition, reconfigure, solve.  Rows (track_cost to 1e-12 relative: another order of summation), states and
    log bit for bit."""
    B, T, n = 4, 3, 12
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    x0 = pkg.problems.wb_ensemble_x0(B, 20241222)
    opt0, opt_rt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4), pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    A = pkg.MultiPhaseDDP(phases, batch=B); M = pkg.MultiPhaseDDP(phases, batch=B)
    epi = A.episode(n, T, keep_log=True); epi.set_grf(MU); epi.set_substeps(4)
    epi.reset(x0); M.set_initial_condition(x0)
    A.solve(opt0); M.solve(opt0)
    dist, kick = mc.cases(pkg, (B,))["D"]
    ident = (list(range(len(phases))), [0] * len(phases))
    smap = sc.step_map(phases, n)
    assert not smap[2].any()      # the tick ends on a lift-off: no reset map inside it and none pending
    state, ic, rows = x0.copy(), x0.copy(), ep.empty_rows(B)
    logX, logU, logY = np.zeros((B, T * n + 1, 36)), np.zeros((B, T * n, 12)), np.zeros((B, T * n, 12))
    for t in range(T):
        epi.advance(dist, kick)
        assert epi.substeps == 4
        sim = pkg.Simulation(M, 1, n, keep_traj=True); sim.set_grf(MU); sim.set_substeps(4)
        sim.run(np.ascontiguousarray(state[:, None]), dist=dataclasses.replace(dist, seed=ep.tick_seed(dist.seed, t)), kick=np.ascontiguousarray(kick[:, None]))
        srows, xf = sim.rows(); extra = sim.extra(); grf, Y = sim.grf(); X, U = sim.traj(); sim.close()
        q, r = ep.step_weights(phases, smap); xr, ur = ep.step_refs(M, smap)
        live0 = rows["end_reason"] == 0
        rows = ep.fold_rows(rows, t, srows[:, 0], X[:, 0], U[:, 0], q, r, xr, ur, extra=extra[:, 0], grf=grf[:, 0], status=M.info_arrays()["status"])
        logX[live0, t * n:(t + 1) * n + 1] = X[live0, 0]; logU[live0, t * n:(t + 1) * n] = U[live0, 0]; logY[live0, t * n:(t + 1) * n] = Y[live0, 0]
        state[live0] = xf[live0, 0]
        live1 = rows["end_reason"] == 0
        erows, ex = epi.rows()
        for f in rows.dtype.names:
            if f != "track_cost":
                assert np.array_equal(erows[f], rows[f]), (t, f, erows[f], rows[f])
        rel = np.abs(erows["track_cost"] - rows["track_cost"]) / np.abs(rows["track_cost"])
        print(f"[sub] episode tick {t}: track_cost {erows['track_cost']}, rel diff to fold_rows {rel.max():.3e}, alive {int(live1.sum())}, n_slip {erows['n_slip']}")
        assert rel.max() <= 1e-12 and np.array_equal(ex, state)
        eX, eU, eY = epi.log()
        assert np.array_equal(eX, logX) and np.array_equal(eU, logU) and np.array_equal(eY, logY)
        assert epi.status() == (t + 1, int(live1.sum()), 0)
        ic[live1] = state[live1]      # (a problem that ended keeps the initial condition of its last whole tick, as in the episode)
        M.set_initial_condition(ic)
        A.reconfigure(phases, *ident); M.reconfigure(phases, *ident)
        A.solve(opt_rt); M.solve(opt_rt)
        for i in range(len(phases)):
            for f in ("K", "XBAR", "UBAR"):
                assert A.field(i, f).tobytes() == M.field(i, f).tobytes(), (t, i, f)
    assert epi.substeps == 4 and np.abs(logY).max() > 1.0
    # S = 4 did act: the same first tick with one substep ends elsewhere
    sim = pkg.Simulation(M, 1, n, keep_traj=True)
    sim.run(np.ascontiguousarray(x0[:, None]), dist=dist, kick=np.ascontiguousarray(kick[:, None]))
    assert np.abs(sim.traj()[0][:, 0] - logX[:, :n + 1]).max() > 1e-3
    sim.close(); epi.close(); A.close(); M.close()


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_substep_refusals_allocation_and_handle(hip_lib):
    lib = pkg._abi.bind_substep(hip_lib)
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(pkg.problems.wb_ensemble_x0(5, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    before = snapshot(s)
    sim = pkg.Simulation(s, 3, 20, keep_traj=True)
    sim.run(xs); first = collect(sim, False)
    v = ctypes.c_int(-7)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_substep_get(sim.s, ctypes.byref(v)) == 0 and v.value == 1
    for bad in (0, -1, 65, 1 << 20):
        assert lib.hsddp_substep_set(sim.s, bad) == EINVAL, bad
    assert lib.hsddp_substep_set(None, 4) == EINVAL and lib.hsddp_substep_get(None, ctypes.byref(v)) == EINVAL and lib.hsddp_substep_get(sim.s, None) == EINVAL
    with pytest.raises(RuntimeError):
        sim.set_substeps(65)
    assert sim.substeps == 1
    sim.run(xs); same_bits(collect(sim, False), first)                                   # the refused calls changed nothing
    assert lib.hsddp_substep_set(sim.s, 1) == 0                                           # one substep on an object that never had more: nothing to do
    assert hip_lib.hsddp_debug_malloc_count() == mallocs
    sim.set_substeps(64); assert sim.substeps == 64
    assert hip_lib.hsddp_debug_malloc_count() == mallocs + 1                             # the trip count's block
    for bad in (0, 65):
        assert lib.hsddp_substep_set(sim.s, bad) == EINVAL and sim.substeps == 64
    sim.set_substeps(3)
    sim.run(xs); three = collect(sim, False)
    sim.set_grf(MU); sim.run(xs); sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.grf()      # first uses allocate their own buffers
    m2 = hip_lib.hsddp_debug_malloc_count()
    sim.set_substeps(5); sim.run(xs); sim.set_substeps(1); sim.run(xs); sim.set_substeps(3); sim.run(xs, dist=Dist(seed=3, u_max=17.0))
    sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.set_grf(0.0); sim.run(xs)
    assert hip_lib.hsddp_debug_malloc_count() == m2                                      # later calls and all runs allocate nothing
    same_bits(collect(sim, False), three)
    assert not np.array_equal(three["X"], first["X"])
    after = snapshot(s)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k                              # the handle is bit for bit what it was
    res = s.simulate(xs, 20, substeps=3)                                                 # the one-off path
    assert res["rows"].tobytes() == three["rows"].tobytes() and np.array_equal(res["x_final"], three["x_final"])
    s.reconfigure(phases, list(range(len(phases))), [0] * len(phases))
    with pytest.raises(RuntimeError):
        sim.run(xs)                                                                       # stale, as without substeps
    assert sim.substeps == 3
    sim.close(); s.close()
