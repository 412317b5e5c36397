"""Contact-force records (include/hsddp_grf.h; kernels k_sim_quad_grf, k_sim_quad_mc_grf, k_sim_quad_mc0_grf of cafe-mpc_amd/csrc/wb_sim.hpp) on
the device: parity with the oracle's forces (tests/grf_common.py), the records changing nothing else a run returns, the three kernels against each
other, consistency of the row with the returned forces under real disturbances, the shapes the quad mapping can get wrong, contained divergence,
refusals, allocation and staleness."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import parity_common as pc
import sim_common as sc
import mc_common as mc
import grf_common as gc

pytestmark = pytest.mark.gpu

EINVAL = -1
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
FLOATS = ("min_fz", "min_cone", "max_fz")
Dist = pkg.sim.Disturbance
NOISY = dict(seed=7, sigma_u=0.2, sigma_q=1e-3, sigma_v=1e-2, u_max=17, fall_height=0.16)


@pytest.fixture(scope="module")
def trot12(oracle_lib, hip_lib):
    """trot12 of tests/test_sim_gpu.py: trot 4 x 12, B = 4 (wb_ensemble_x0(4, 20241222)), 3 AL x 4 DDP on the oracle and on the device, R = 8 samples
    (sigma 0.02 / 0.2, seed 20241222) around Xbar[0].  The oracle's forces of a window are computed once per window length and shared."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, pkg.problems.wb_ensemble_x0(4, 20241222))
    opt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4)
    so.solve(opt); sg.solve(opt)
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    cache = {}

    def yref(n):
        if n not in cache:
            cache[n] = gc.oracle_forces(so, pkg.mhpc_ddp_setting(MS=0), xs, sc.step_map(phases, n))
            cache[n].setflags(write=False)
        return cache[n]
    yield phases, sg, xs, yref
    so.close(); sg.close()


def same_but_records(a, b):
    """Everything a run returned before the records existed, bit for bit."""
    for f in ("x_final", "X", "U"):
        if f in a or f in b:
            assert np.array_equal(a[f], b[f]), f
    assert a["rows"].tobytes() == b["rows"].tobytes()
    assert ("extra" in a) == ("extra" in b)
    if "extra" in a:
        assert a["extra"].tobytes() == b["extra"].tobytes()


def own_rows_agree(tag, res, contact, mu, fz_min):
    """The returned row against sim.grf_rows of the returned forces over the steps the sample was alive at: floats to 1e-12 x the force scale (a
    fused multiply-add in cone), counters equal - the returned forces keep 1e-9 N from every threshold, which is asserted."""
    fb = res["rows"]["first_bad"]
    own = pkg.sim.grf_rows(res["Y"], contact, mu, fz_min, first_bad=fb)
    scale = max(1.0, float(np.abs(res["Y"]).max()))
    mcone, mfz = gc.margins(res["Y"], contact, mu, fz_min, first_bad=fb)
    err = max(float(np.abs(res["grf"][f] - own[f]).max()) for f in FLOATS)
    print(f"[grf] {tag}: row against grf_rows(own Y): |diff| = {err:.3e}, scale {scale:.3e}, bound {1e-12 * scale:.3e}; own margins {mcone:.3e} / {mfz:.3e} N; "
          f"slipping samples {int((own['first_slip'] >= 0).sum())} of {own.size}, n_slip {int(own['n_slip'].sum())}")
    assert np.isfinite(res["Y"]).all() and err <= 1e-12 * scale, tag
    assert mcone >= 1e-9 and mfz >= 1e-9, tag
    assert np.array_equal(res["grf"]["first_slip"], own["first_slip"]) and np.array_equal(res["grf"]["n_slip"], own["n_slip"]), tag
    gc.assert_swing_is_zero(tag, res["Y"], contact)


@pytest.mark.parametrize("n_steps", [13, 48])
def test_grf_parity_trot_windows(trot12, n_steps):
    """One step past the lift-off boundary (the stance set changes); across both touchdowns.  The GPU and the oracle each simulate their own solved
    policy, as test_sim_parity_trot_windows does.  mu = 0.6 and mu = 0.3, fz_min = 0: forces, floats and EQUAL counters (grf_common.compare_records;
    margins of the reference: tests/test_grf_host.py).  The lean run without keep_traj gives the same row bytes."""
    phases, sg, xs, yref = trot12
    smap = sc.step_map(phases, n_steps)
    contact = gc.contact_of(phases, smap)
    for mu in (0.6, 0.3):
        res = sg.simulate(xs, n_steps, keep_traj=True, grf=(mu, 0.0))
        assert res["Y"].shape == (4, 8, n_steps, 12) and res["grf"].shape == (4, 8) and res["grf"].dtype == pkg._abi.GRF_ROW_DTYPE
        ref = gc.compare_records(f"gpu n={n_steps} mu={mu}", pkg, res["grf"], res["Y"], yref(n_steps), contact, mu, 0.0)
        if mu == 0.6:
            assert int((ref["first_slip"] >= 0).sum()) == 16 and int((ref["min_fz"] < 0).sum()) == 1
        lean = sg.simulate(xs, n_steps, grf=(mu, 0.0))
        assert set(lean) == {"rows", "x_final", "grf"} and lean["grf"].tobytes() == res["grf"].tobytes() and lean["rows"].tobytes() == res["rows"].tobytes()


CASES = {"plain": (None, False), "noisy": (Dist(kick_step=10, **NOISY), True), "umax": (Dist(seed=7, u_max=17), False)}


@pytest.mark.parametrize("case", list(CASES))
def test_grf_records_change_nothing_else(trot12, hip_lib, case):
    """n = 48, keep_traj: rows, x_final, X, U (and extra of the disturbed runs) bit-identical with the records on and off - on ONE object, so after
    set_grf(0) the run is again the original, and hsddp_grf_get is then refused.  plain: k_sim_quad_grf against k_sim_quad; noisy (with a kick):
    k_sim_quad_mc_grf against k_sim_quad_mc; umax: k_sim_quad_mc0_grf against k_sim_quad_mc0."""
    phases, sg, xs, yref = trot12
    d, kicked = CASES[case]
    kick = mc.kick_y(xs.shape[:2], 0.3) if kicked else None
    lib = pkg._abi.bind_grf(hip_lib)

    def collect(sim):
        rows, xf = sim.rows(); X, U = sim.traj()
        out = dict(rows=rows, x_final=xf, X=X, U=U)
        if d is not None:
            out["extra"] = sim.extra()
        return out
    sim = pkg.Simulation(sg, 8, 48, keep_traj=True)
    sim.run(xs, dist=d, kick=kick); off = collect(sim)
    buf = np.zeros((4, 8), dtype=pkg._abi.GRF_ROW_DTYPE)
    assert lib.hsddp_grf_get(sim.s, 0, 4, buf.ctypes.data, None) == EINVAL          # never switched on
    sim.set_grf(0.6)
    sim.run(xs, dist=d, kick=kick); on = collect(sim)
    g, Y = sim.grf()
    same_but_records(on, off)
    assert (g["max_fz"] > 1.0).all() and np.abs(Y).max() > 1.0                          # (and the records were taken)
    sim.set_grf(0.0)
    sim.run(xs, dist=d, kick=kick); again = collect(sim)
    same_but_records(again, off)
    assert lib.hsddp_grf_get(sim.s, 0, 4, buf.ctypes.data, None) == EINVAL          # the last run was made with the records off
    with pytest.raises(RuntimeError):
        sim.grf()
    sim.close()


def test_grf_three_kernels_agree(trot12):
    """The plain run with records (k_sim_quad_grf, held to the oracle by the parity test) against three disturbed runs that reduce to it by
    construction: u_max = 1e9 alone (k_sim_quad_mc0_grf: the walk without the generator, clipping nothing); sigma_u = 1e-300 (k_sim_quad_mc_grf:
    every torque normal drawn, nothing representable added); all three sigmas 1e-300 (all 48 normals drawn).  The last two differ only in their
    sigmas: a disagreement in one and not the other separates the torque draws from the estimate draws.  Forces and floats at the tolerance of the
    parity test, counters equal."""
    phases, sg, xs, yref = trot12
    smap = sc.step_map(phases, 48)
    contact = gc.contact_of(phases, smap)
    plain = sg.simulate(xs, 48, keep_traj=True, grf=(0.6, 0.0))
    scale = max(1.0, float(np.abs(plain["Y"]).max()))
    for tag, d in (("u_max 1e9", Dist(seed=7, u_max=1e9)), ("sigma_u 1e-300", Dist(seed=7, sigma_u=1e-300)),
                   ("all sigmas 1e-300", Dist(seed=7, sigma_u=1e-300, sigma_q=1e-300, sigma_v=1e-300))):
        res = sg.simulate(xs, 48, keep_traj=True, dist=d, grf=(0.6, 0.0))
        assert (res["extra"]["n_sat"] == 0).all() and (res["extra"]["first_fall"] == -1).all()
        sc.close(f"{tag} X", res["X"], plain["X"]); sc.close(f"{tag} U", res["U"], plain["U"])
        gc.compare_records(tag, pkg, res["grf"], res["Y"], plain["Y"], contact, 0.6, 0.0)      # (reference: the plain run's forces)
        for f in FLOATS:
            sc.close(f"{tag} {f} against the plain row", res["grf"][f], plain["grf"][f], scale=scale)
        assert np.array_equal(res["grf"]["first_slip"], plain["grf"]["first_slip"]) and np.array_equal(res["grf"]["n_slip"], plain["grf"]["n_slip"]), tag


def test_grf_row_is_consistent_with_the_forces_under_disturbances(trot12):
    """The noisy run with a push, keep_traj: the returned row is grf_rows of the returned Y."""
    phases, sg, xs, yref = trot12
    contact = gc.contact_of(phases, sc.step_map(phases, 48))
    for mu, fz_min in ((0.6, 0.0), (0.4, 5.0)):
        res = sg.simulate(xs, 48, keep_traj=True, dist=Dist(kick_step=10, **NOISY), kick=mc.kick_y(xs.shape[:2], 0.3), grf=(mu, fz_min))
        own_rows_agree(f"noisy mu={mu} fz_min={fz_min}", res, contact, mu, fz_min)
        assert (res["grf"]["first_slip"] >= 0).any()


def test_grf_partial_wave_with_quads_of_three_problems(oracle_lib, hip_lib):
    """B = 3, R = 3, trot 4 x 6, n = 20: nine quads - one partial wave, with quads of three problems in it.  Reference: the window walked with the
    oracle's model probes and the device handle's own policy (grf_common.oracle_walk_forces), so that a quad reading another problem's policy
    shows; forces and floats at the rollout tolerance, counters against the row of the device's own forces."""
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=3); s.set_initial_condition(pkg.problems.wb_ensemble_x0(3, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    smap = sc.step_map(phases, 20)
    contact = gc.contact_of(phases, smap)
    Yref = gc.oracle_walk_forces(oracle_lib, phases, mc.policy_of(s), smap, xs)
    res = s.simulate(xs, 20, keep_traj=True, grf=(0.6, 0.0))
    assert (res["rows"]["first_bad"] == -1).all()
    sc.close("3 x 3 Y", res["Y"], Yref)
    ref = pkg.sim.grf_rows(Yref, contact, 0.6, 0.0)
    for f in FLOATS:
        sc.close(f"3 x 3 {f}", res["grf"][f], ref[f], scale=max(1.0, float(np.abs(Yref).max())))
    own_rows_agree("3 x 3", res, contact, 0.6, 0.0)
    # and against the reference walk, counters included (its margins, measured with the oracle: min |cone| 0.15 N, min |fz| 2.4 N against 4.7e-4 N
    # needed - asserted by compare_records): a counter written to the wrong quad shows here
    gc.compare_records("3 x 3 against the walk", pkg, res["grf"], res["Y"], Yref, contact, 0.6, 0.0)
    assert len({res["Y"][b, r].tobytes() for b in range(3) for r in range(3)}) == 9
    s.close()


def test_grf_samples_are_independent(trot12):
    """R = 1 against R = 8 (another place in the wave), n = 24: the same row and Y bytes per sample, as test_sim_samples_are_independent."""
    phases, sg, xs, yref = trot12
    full = sg.simulate(xs, 24, keep_traj=True, grf=(0.6, 0.0))
    for r in (0, 3, 7):
        one = sg.simulate(np.ascontiguousarray(xs[:, r:r + 1]), 24, keep_traj=True, grf=(0.6, 0.0))
        assert np.array_equal(one["Y"][:, 0], full["Y"][:, r]) and one["grf"][:, 0].tobytes() == full["grf"][:, r].tobytes(), r


def test_grf_divergence_is_contained(trot12):
    """The case of test_sim_divergence_is_contained: sample (2, 5) fails the divergence test at step 0.  It was alive when step 0 began, so its
    record is exactly that of step 0 alone - the forces computed from the kept state - and not the empty row; every other sample's row and forces
    are bit-identical to the clean run."""
    phases, sg, xs, yref = trot12
    contact = gc.contact_of(phases, sc.step_map(phases, 48))
    clean = sg.simulate(xs, 48, keep_traj=True, grf=(0.6, 0.0))
    x = xs.copy(); x[2, 5, 18] = 1e7
    res = sg.simulate(x, 48, keep_traj=True, grf=(0.6, 0.0))
    assert res["rows"]["first_bad"][2, 5] == 0 and (clean["rows"]["first_bad"] == -1).all()
    got, Y0 = res["grf"][2, 5], res["Y"][2, 5, :1]
    own = pkg.sim.grf_rows(Y0, contact[:1], 0.6, 0.0)
    scale = max(1.0, float(np.abs(Y0).max()))
    print(f"[grf] diverged sample: row {got}, of step 0 alone {own}, force scale {scale:.3e}")
    assert np.isfinite(Y0).all() and np.isfinite(got["max_fz"]) and np.isfinite(got["min_fz"])          # not the empty row
    for f in FLOATS:
        assert abs(got[f] - own[f]) <= 1e-12 * scale, f
    assert gc.margins(Y0, contact[:1], 0.6, 0.0)[0] >= 1e-9 * scale and got["first_slip"] == own["first_slip"] and got["n_slip"] == own["n_slip"]
    assert got["n_slip"] <= int(contact[0].sum()) and got["first_slip"] in (-1, 0)                      # the stance feet of one step
    keep = np.ones((4, 8), dtype=bool); keep[2, 5] = False
    assert np.array_equal(res["Y"][keep], clean["Y"][keep]) and res["grf"][keep].tobytes() == clean["grf"][keep].tobytes()
    assert res["rows"][keep].tobytes() == clean["rows"][keep].tobytes()


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_grf_refusals_allocation_and_staleness(hip_lib):
    lib = pkg._abi.bind_grf(hip_lib)
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(pkg.problems.wb_ensemble_x0(5, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    before = snapshot(s)
    sim = pkg.Simulation(s, 3, 20, keep_traj=True)
    lean = pkg.Simulation(s, 3, 20)
    rows = np.zeros((5, 3), dtype=pkg._abi.GRF_ROW_DTYPE); Y = np.zeros((5, 3, 20, 12))
    cd = ctypes.c_double
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_grf_set(None, cd(0.6), cd(0.0)) == EINVAL
    for mu, fz in ((-0.1, 0.0), (np.nan, 0.0), (np.inf, 0.0), (0.6, -1.0), (0.6, np.nan), (0.6, np.inf)):
        assert lib.hsddp_grf_set(sim.s, cd(mu), cd(fz)) == EINVAL, (mu, fz)
    sim.run(xs)
    assert lib.hsddp_grf_get(sim.s, 0, 5, rows.ctypes.data, None) == EINVAL             # the refused calls switched nothing on
    assert lib.hsddp_grf_set(sim.s, cd(0.0), cd(0.0)) == 0                               # off on an object that never had them on: nothing to do
    assert hip_lib.hsddp_debug_malloc_count() == mallocs
    sim.set_grf(0.6)                                                                      # rows, Y and the thresholds
    assert hip_lib.hsddp_debug_malloc_count() == mallocs + 3
    lean.set_grf(0.6)                                                                     # rows and the thresholds
    assert hip_lib.hsddp_debug_malloc_count() == mallocs + 5
    assert lib.hsddp_grf_get(sim.s, 0, 5, rows.ctypes.data, None) == EINVAL             # on, but the last run was made with the records off
    sim.run(xs); lean.run(xs)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    first, Y1 = sim.grf()
    for b0, nb in ((-1, 1), (0, 0), (0, 6), (5, 1), (4, 2)):
        assert lib.hsddp_grf_get(sim.s, b0, nb, rows.ctypes.data, None) == EINVAL, (b0, nb)
    assert lib.hsddp_grf_get(sim.s, 0, 5, None, None) == EINVAL and lib.hsddp_grf_get(None, 0, 5, rows.ctypes.data, None) == EINVAL
    assert lib.hsddp_grf_get(lean.s, 0, 5, rows.ctypes.data, Y.ctypes.data) == EINVAL    # created without keep_traj
    assert lib.hsddp_grf_set(sim.s, cd(-1.0), cd(0.0)) == EINVAL
    assert lib.hsddp_grf_get(lean.s, 0, 5, rows.ctypes.data, None) == 0 and rows.tobytes() == first.tobytes() and lean.grf().tobytes() == first.tobytes()
    assert lib.hsddp_grf_get(sim.s, 3, 2, rows.ctypes.data, Y.ctypes.data) == 0 and rows[:2].tobytes() == first[3:].tobytes() and np.array_equal(Y[:2], Y1[3:])
    sim.set_grf(0.6); sim.set_grf(0.3, 1.0); sim.run(xs); second, Y2 = sim.grf()         # a second switching-on call and warm runs allocate nothing
    sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.grf()      # (the first disturbed run allocates its own buffers)
    assert np.array_equal(Y1, Y2) and (second["n_slip"] >= first["n_slip"]).all() and (second["n_slip"] > first["n_slip"]).any()
    assert np.array_equal(second["min_fz"], first["min_fz"]) and np.array_equal(second["max_fz"], first["max_fz"])
    m2 = hip_lib.hsddp_debug_malloc_count()
    sim.set_grf(0.6); sim.run(xs); sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.grf(); lean.run(xs); lean.grf()
    assert hip_lib.hsddp_debug_malloc_count() == m2 and m2 == mallocs + 2               # (+ 2: the extras and the switches of the first disturbed run)
    after = snapshot(s)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k                              # the handle is bit for bit what it was
    s.reconfigure(phases, list(range(len(phases))), [0] * len(phases))
    with pytest.raises(RuntimeError):
        sim.run(xs)                                                                       # stale, as without records
    sim.set_grf(0.6)
    with pytest.raises(RuntimeError):
        sim.run(xs)
    sim.close(); lean.close(); s.close()
