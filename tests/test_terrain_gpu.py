"""Terrain height maps and early swing-foot touchdown (include/hsddp_terrain.h; kernels k_sim_quad_ter, k_sim_quad_mc_ter, k_sim_quad_mc0_ter of
cafe-mpc_amd/csrc/hsddp_ter.hip) on the device: the cases of tests/ter_common.py against the reference walk with the device's own policy, flat ground
against the run without the terrain, a map per sample, feet outside the grid on a partial wave, contained divergence, toggling and the prefix property,
refusals and allocation, and episodes with (F, E) carried from tick to tick."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import sim_common as sc
import mc_common as mc
import grf_common as gc
import uni_common as un
import ter_common as tc

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -1, -3
MU = 0.6
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
Dist = pkg.sim.Disturbance
Terrain = pkg.sim.Terrain
ep = pkg.episode
INTS = ("first_release", "n_release", "n_land", "n_free", "free_final")


@pytest.fixture(scope="module")
def trot12(oracle_lib, hip_lib):
    """trot12 of tests/test_contact_gpu.py: trot 4 x 12, B = 4, 3 AL x 4 DDP, R = 8 samples around Xbar[0]; the policy rows of the DEVICE handle."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    sg = pkg.MultiPhaseDDP(phases, batch=4)
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); sg.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(sg.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, sg, xs, mc.policy_of(sg)
    sg.close()


def same_bits(a, b, but=()):
    assert set(a) == set(b)
    for f in a:
        if f not in but:
            assert a[f].tobytes() == b[f].tobytes(), f


def test_flat_terrain_is_the_contact_run(trot12):
    """Case 1: H = 0, early = 0, S = 3 on the flight case (k_sim_quad_mc0_ter) against the run without the terrain (k_sim_quad_mc0_uni): the integer
    rows are equal, the floats agree within the tolerance (bit-identity is printed), every new counter is 0."""
    phases, sg, xs, pol = trot12
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "flat", xs)
    res = tc.library_run(pkg, sg, x0, 48, 3, fz_rel, zg, ter, d, k, MU)
    base = un.library_run(pkg, sg, x0, 48, 3, fz_rel, zg, d, k, MU)
    t = res.pop("terrain")
    same = all(res[f].tobytes() == base[f].tobytes() for f in base)
    print(f"[ter] gpu flat: bit-identical to the run without the terrain: {same}")
    assert base["contact"]["n_release"].sum() > 0 and base["contact"]["n_land"].sum() > 0
    for f in INTS:
        assert np.array_equal(res["contact"][f], base["contact"][f]), f
    assert np.array_equal(res["rows"]["first_bad"], base["rows"]["first_bad"]) and np.array_equal(res["grf"]["n_slip"], base["grf"]["n_slip"]) and np.array_equal(res["extra"], base["extra"])
    for f in ("X", "U", "x_final", "Y"):
        sc.close(f"gpu flat {f}", res[f], base[f], scale=max(1.0, float(np.abs(base[f]).max())))
    sc.close("gpu flat max_lift", res["contact"]["max_lift"], base["contact"]["max_lift"], scale=1.0)
    assert (t["first_early"] == -1).all() and not t["n_early"].any() and not t["n_early_release"].any() and not t["n_held"].any() and not t["early_final"].any()
    assert (t["max_pen"] >= 0.0).all() and not t["max_pen"][base["contact"]["n_land"] == 0].any()


@pytest.mark.parametrize("case,S", tc.CASES)
def test_terrain_cases_match_the_reference(trot12, oracle_lib, case, S):
    """Cases 2 - 5 of ter_common.case_setup: the block at S = 1 and 4 (k_sim_quad_mc0_ter), a map per sample under noise (k_sim_quad_mc_ter), feet
    outside the grid on a partial wave at S = 5 and the contained divergence, against the reference walk; non-vacuity and the cap of one left-out
    sample are asserted on the reference first."""
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
    B = x0.shape[0]
    if B == 4:
        s, polB = sg, pol
    else:      # fewer problems: a handle of that batch with the same problems, its own policy rows
        s = pkg.MultiPhaseDDP(phases, batch=B)
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)[:B]); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
        polB = mc.policy_of(s)
    ref = tc.oracle_walk_ter(pkg, oracle_lib, phases, polB, smap, x0, S, fz_rel, zg, ter, d, k)
    tc.assert_case_is_not_vacuous(case, ref, ter)
    if case == "maps":
        tc.assert_pit_samples_land_lower(ref, ter)
    res = tc.library_run(pkg, s, x0, 48, S, fz_rel, zg, ter, d, k, MU)
    assert res["terrain"].shape == x0.shape[:2] and res["contact"].shape == x0.shape[:2]
    tc.compare_case(f"gpu {case} S={S}", pkg, res, ref, mc.xbar_window(polB, smap), MU, 0.0, fz_rel)
    if case == "maps":      # the samples of map 0 equal a one-map run of their own, bit for bit
        alone = tc.library_run(pkg, s, x0, 48, S, fz_rel, zg, Terrain(H=ter.grid()[:1], early=True, w_td=ter.w_td), d, k, MU)
        m0 = np.asarray(ter.map_of) == 0
        for f in res:
            assert res[f][m0].tobytes() == alone[f][m0].tobytes(), f
        assert not np.array_equal(res["x_final"][~m0], alone["x_final"][~m0])
    if case == "divergence":
        assert res["rows"]["first_bad"][1, 1] == 5 and np.array_equal(res["X"][1, 1, 6:], np.broadcast_to(res["x_final"][1, 1], (43, 36)))
        sc.close("kept state", res["x_final"][1, 1], ref["X"][1, 1, -1], scale=float(np.abs(ref["X"][1, 1, -1]).max()))
    if s is not sg:
        s.close()


def collect(sim, disturbed, contact, terrain=False):
    rows, xf = sim.rows(); X, U = sim.traj()
    out = dict(rows=rows, x_final=xf, X=X, U=U)
    if disturbed:
        out["extra"] = sim.extra()
    if contact:
        out["contact"] = sim.contact_rows()
    if terrain:
        out["terrain"] = sim.terrain_rows()
    return out


def test_toggling_dormancy_and_prefix(trot12):
    """Case 6 on one object, block case, S = 4: terrain on, off, on - the off run is bit-identical to an object that never had a terrain, the two on
    runs are bit-identical; with the contact rule off and the terrain on a run has the bits of a fresh object (the terrain is dormant); and the
    24-step run with the terrain on is the first 24 steps of the 48-step one."""
    phases, sg, xs, pol = trot12
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "block", xs)
    fresh = pkg.Simulation(sg, 8, 48, keep_traj=True); fresh.set_substeps(4)
    fresh.run(x0, dist=d, kick=k); want_plain = collect(fresh, True, False)
    fresh.set_contact(fz_rel, zg); fresh.run(x0, dist=d, kick=k); want_uni = collect(fresh, True, True); fresh.close()
    sim = pkg.Simulation(sg, 8, 48, keep_traj=True); sim.set_substeps(4)
    assert sim.terrain[0] is False and sim.terrain[1]["nx"] == 0
    sim.set_terrain(ter)                      # the contact rule is off: dormant
    on, par = sim.terrain
    assert on and (par["nx"], par["ny"], par["n_maps"], par["early"], par["x0"], par["cx"], par["w_td"]) == (2, 1, 1, 1, -9.85, 10.0, tc.W_TD)
    sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, False), want_plain)
    with pytest.raises(RuntimeError):
        sim.terrain_rows()                    # the last run had the terrain dormant
    sim.set_contact(fz_rel, zg)
    sim.run(x0, dist=d, kick=k); on1 = collect(sim, True, True, True)
    sim.clear_terrain(); assert sim.terrain[0] is False
    sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, True), want_uni)
    with pytest.raises(RuntimeError):
        sim.terrain_rows()
    sim.set_terrain(ter)
    sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, True, True), on1)
    assert on1["terrain"]["n_early"].sum() > 0 and not np.array_equal(on1["X"], want_uni["X"])
    sim.clear_contact()
    sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, False), want_plain)
    sim.close()
    d16 = dataclasses.replace(d, kick_step=16)      # inside both windows
    long = tc.library_run(pkg, sg, x0, 48, 4, fz_rel, zg, ter, d16, k, MU)
    short = tc.library_run(pkg, sg, x0, 24, 4, fz_rel, zg, ter, d16, k, MU)
    assert short["terrain"]["n_early"].sum() > 0
    assert np.array_equal(long["X"][:, :, :24], short["X"][:, :, :24]) and np.array_equal(long["U"][:, :, :24], short["U"]) and np.array_equal(long["Y"][:, :, :24], short["Y"])
    assert np.array_equal(long["X"][:, :, 24, :18], short["X"][:, :, 24, :18])      # (entry 24 of the long run lies behind a reset map: positions stay)


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_terrain_refusals_allocation_and_handle(hip_lib):
    """Case 7: every refusal of the header with nothing changed, hsddp_terrain_get_params, the allocation count, the handle left as it was, and the
    one-off simulate(..., terrain=) path equal to the object path."""
    lib = pkg._abi.bind_terrain(hip_lib)
    TP = pkg._abi.TerrainParams
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(pkg.problems.wb_ensemble_x0(5, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    before = snapshot(s)
    sim = pkg.Simulation(s, 3, 20, keep_traj=True)
    sim.set_contact(-3.0, 0.0)
    sim.run(xs); first = collect(sim, False, True)
    H = np.zeros((2, 3, 4)); H[1] = 0.01
    mo = (np.arange(15).reshape(5, 3) % 2).astype(np.int32)
    good = dict(nx=4, ny=3, n_maps=2, early=1, x0=-0.5, y0=-0.5, cx=0.25, cy=0.3, w_td=0.05)
    par = lambda **kw: TP(**{**good, **kw})
    setc = lambda t, h=H, m=mo, on=1: lib.hsddp_terrain_set(sim.s, on, None if t is None else ctypes.byref(t), None if h is None else h.ctypes.data, None if m is None else m.ctypes.data)
    on, got = ctypes.c_int(-7), TP()
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_terrain_get_params(sim.s, ctypes.byref(on), ctypes.byref(got)) == 0 and (on.value, got.nx, got.ny, got.n_maps, got.early, got.cx, got.w_td) == (0, 0, 0, 0, 0, 0.0, 0.0)
    assert setc(None) == EINVAL and setc(par(), h=None) == EINVAL and lib.hsddp_terrain_set(None, 1, ctypes.byref(par()), H.ctypes.data, None) == EINVAL
    assert lib.hsddp_terrain_set(None, 0, None, None, None) == EINVAL
    for kw in (dict(x0=np.nan), dict(y0=np.inf), dict(cx=np.nan), dict(cy=-np.inf), dict(w_td=np.nan), dict(cx=0.0), dict(cy=-0.1), dict(w_td=-1e-9),
               dict(nx=0), dict(nx=1025), dict(ny=0), dict(ny=1025), dict(n_maps=0), dict(n_maps=4097)):
        assert setc(par(**kw), h=np.zeros(8)) == EINVAL, kw      # (refused before the grid is read)
    assert setc(par(nx=1024, ny=1024, n_maps=5), h=np.zeros(8)) == EINVAL      # 5 x 2^20 cells > 2^22
    Hn = H.copy(); Hn[1, 2, 3] = np.nan
    Hi = H.copy(); Hi[0, 0, 0] = np.inf
    assert setc(par(), h=Hn) == EINVAL and setc(par(), h=Hi) == EINVAL
    for bad in (2, -1):
        m2 = mo.copy(); m2[4, 2] = bad
        assert setc(par(), m=m2) == EINVAL
    assert lib.hsddp_terrain_get_params(None, ctypes.byref(on), ctypes.byref(got)) == EINVAL and lib.hsddp_terrain_get_params(sim.s, None, ctypes.byref(got)) == EINVAL
    assert lib.hsddp_terrain_get_params(sim.s, ctypes.byref(on), None) == EINVAL
    rows = np.zeros((5, 3), dtype=pkg._abi.TERRAIN_ROW_DTYPE)
    assert lib.hsddp_terrain_get(sim.s, 0, 5, rows.ctypes.data) == EINVAL      # no run with the terrain yet
    assert setc(None, None, None, on=0) == 0                                   # off on an object that never had it on: nothing to do
    assert hip_lib.hsddp_debug_malloc_count() == mallocs and sim.terrain[0] is False
    sim.run(xs); same_bits(collect(sim, False, True), first)                   # the refused calls changed nothing
    ter = Terrain(H=H, x0=-0.5, y0=-0.5, cx=0.25, cy=0.3, early=True, w_td=0.05, map_of=mo)
    sim.set_terrain(ter)
    m1 = hip_lib.hsddp_debug_malloc_count(); assert m1 > mallocs               # the first on allocates
    assert setc(par(cx=0.0)) == EINVAL and setc(par(), h=Hn) == EINVAL
    onp, p = sim.terrain
    assert onp and p == good
    sim.run(xs); one = collect(sim, False, True, True)
    assert lib.hsddp_terrain_get(sim.s, 0, 5, None) == EINVAL and lib.hsddp_terrain_get(sim.s, 3, 3, rows.ctypes.data) == EINVAL and lib.hsddp_terrain_get(sim.s, -1, 2, rows.ctypes.data) == EINVAL
    assert lib.hsddp_terrain_get(None, 0, 5, rows.ctypes.data) == EINVAL
    assert np.array_equal(sim.terrain_rows(1, 2), one["terrain"][1:3])
    sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.set_grf(MU); sim.run(xs); sim.set_substeps(3); sim.run(xs)      # first uses of the others
    m2 = hip_lib.hsddp_debug_malloc_count()
    sim.set_terrain(Terrain(H=H[:1, :2, :2], cx=0.5, cy=0.5)); sim.run(xs)     # a smaller grid: the block that is there holds it
    sim.clear_terrain(); sim.run(xs); sim.set_terrain(ter); sim.set_substeps(1); sim.set_grf(0.0); sim.run(xs)
    again = collect(sim, False, True, True)
    sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.terrain_rows()
    assert hip_lib.hsddp_debug_malloc_count() == m2                            # no run allocates, nor a set call whose grid fits
    same_bits(again, one)
    sim.set_terrain(Terrain(H=np.zeros((3, 4, 4)), cx=0.5, cy=0.5)); assert hip_lib.hsddp_debug_malloc_count() == m2 + 1      # the grid grows: one block
    sim.run(xs); assert hip_lib.hsddp_debug_malloc_count() == m2 + 1
    after = snapshot(s)
    for kf in before:
        assert before[kf].tobytes() == after[kf].tobytes(), kf                 # the handle is bit for bit what it was
    res = s.simulate(xs, 20, keep_traj=True, contact=(-3.0, 0.0), terrain=ter)  # the one-off path
    same_bits(res, one)
    sim.close(); s.close()


def test_one_tick_episode_is_the_run(trot12):
    """Case 8a: one sample per problem, 23 steps (the first swing phase of the window, up to the knot before its touchdown), S = 4, the contact rule
    and the block terrain on through hsddp_episode_sim: rows, state, log, contact and terrain rows bit for bit those of hsddp_mc_run on a simulation
    object (early touchdowns inside the tick and a swing foot held at its end, asserted)."""
    phases, sg, xs, pol = trot12
    n = 23
    x1 = np.ascontiguousarray(xs[:, 0])
    d = Dist(seed=mc.SEED, u_max=8.0, kick_step=4)
    k = np.zeros((4, 36)); k[:, 20] = 0.05
    ter = tc.terrain_of(pkg, "block", (4, 1))
    sim = pkg.Simulation(sg, 1, n, keep_traj=True); sim.set_substeps(4); sim.set_grf(MU); sim.set_contact(un.FZ_REL, 0.0); sim.set_terrain(ter)
    sim.run(np.ascontiguousarray(x1[:, None]), dist=d, kick=np.ascontiguousarray(k[:, None]))
    srows, xf = sim.rows(); X, U = sim.traj(); g, Y = sim.grf(); c = sim.contact_rows(); t = sim.terrain_rows(); sim.close()
    assert (t["n_early"] > 0).any() and (t["early_final"] > 0).any()
    e = sg.episode(n, 1, keep_log=True); e.set_substeps(4); e.set_grf(MU); e.set_contact(un.FZ_REL, 0.0); e.set_terrain(ter)
    e.reset(x1); e.advance(d, k)
    rows, x_now = e.rows(); eX, eU, eY = e.log()
    for f in ("dev_q", "dev_v", "min_height", "max_torque"):
        assert np.array_equal(rows[f], srows[f][:, 0]), f
    for f in ("min_fz", "min_cone", "max_fz", "n_slip", "first_slip"):
        assert np.array_equal(rows[f], g[f][:, 0]), f
    assert np.array_equal(x_now, xf[:, 0]) and np.array_equal(eX, X[:, 0]) and np.array_equal(eU, U[:, 0]) and np.array_equal(eY, Y[:, 0])
    assert e.contact_rows().tobytes() == c[:, 0].tobytes() and e.terrain_rows().tobytes() == t[:, 0].tobytes()
    e.close()
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222))


def test_three_tick_episode_carries_f_and_e(hip_lib, oracle_lib):
    """Case 8b: a trot of 4 x 12 knots that starts in a swing phase (ter_common.episode_phases), B = 4, n_exec = 11, three ticks with hsddp_reconfigure and a solve between them, S = 4, torque limit, the block terrain.
    A tick of 11 steps ends one step before a phase's last knot, where swing feet that met the block are held (a robot ends a tick with E non-empty:
    asserted).  Every tick is compared with the reference walked from the episode's state before the tick, with the policy read from the handle and the
    REFERENCE's (F, E) handed from tick to tick.  hsddp_episode_reset clears E."""
    B, T, n = 4, 3, 11
    phases = tc.episode_phases(pkg)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241222)
    opt0, opt_rt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4), pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    A = pkg.MultiPhaseDDP(phases, batch=B)
    ter = tc.terrain_of(pkg, "episode", (B, 1))
    epi = A.episode(n, T, keep_log=True); epi.set_grf(MU); epi.set_substeps(4); epi.set_contact(un.FZ_REL, 0.0); epi.set_terrain(ter)
    epi.reset(x0); A.solve(opt0)
    dist = Dist(seed=mc.SEED, u_max=8.0, kick_step=0)
    kick = np.zeros((B, 36))      # (no push: a zero kick at step 0)
    ident = (list(range(len(phases))), [0] * len(phases))
    smap = sc.step_map(phases, n)
    state, F, E = x0.copy(), np.zeros((B, 1, 4), dtype=bool), np.zeros((B, 1, 4), dtype=bool)
    held_over = False
    for t in range(T):
        pol = mc.policy_of(A)
        ref = tc.oracle_walk_ter(pkg, oracle_lib, phases, pol, smap, np.ascontiguousarray(state[:, None]), 4, un.FZ_REL, 0.0, ter,
                                 dataclasses.replace(dist, seed=ep.tick_seed(dist.seed, t)), None, F0=F, E0=E)
        live0 = epi.rows()[0]["end_reason"] == 0
        epi.advance(dist, kick)
        erows, x_now = epi.rows(); c = epi.contact_rows(); tr = epi.terrain_rows()
        near = un.near_samples(f"episode tick {t}", ref)[:, 0]
        ok = live0 & ~near & (ref["first_bad"][:, 0] < 0)
        print(f"[ter] episode tick {t}: early_final {tr['early_final']}, n_early {tr['n_early']}, n_held {tr['n_held']}, free_final {c['free_final']}, compared {int(ok.sum())} of {B}")
        assert ok.sum() >= B - 1
        for f in INTS:
            assert np.array_equal(c[f][ok], ref["rows"][f][ok, 0]), (t, f, c[f], ref["rows"][f][:, 0])
        for f in tc.INTS_T:
            assert np.array_equal(tr[f][ok], ref["trows"][f][ok, 0]), (t, f, tr[f], ref["trows"][f][:, 0])
        sc.close(f"episode tick {t} state", x_now[ok], ref["X"][ok, 0, -1])
        if t > 0 and (E[:, 0].any(axis=-1) & ok).any():
            held_over = held_over or bool((ref["trows"]["n_held"][:, 0] > 0)[E[:, 0].any(axis=-1) & ok].any())      # the E of the tick before did act in this one
        state, F, E = x_now, ref["F"], ref["E"]
        if t == 0:
            assert (E[:, 0].any(axis=-1) & ok).any(), "no robot ends tick 0 with a swing foot held"
        A.reconfigure(phases, *ident); A.solve(opt_rt)
    assert held_over
    # hsddp_episode_reset clears E: a tick that leaves a foot held, reset, the same tick again under the same policy - the same bits, which a carried
    # E would change; and that tick is the reference's with E empty
    epi.reset(x0); epi.advance(dist, kick)
    x_a, t_a = epi.rows()[1].copy(), epi.terrain_rows().copy()
    assert t_a["early_final"].any()
    epi.reset(x0); epi.advance(dist, kick)
    assert np.array_equal(epi.rows()[1], x_a) and epi.terrain_rows().tobytes() == t_a.tobytes()
    ref = tc.oracle_walk_ter(pkg, oracle_lib, phases, mc.policy_of(A), smap, np.ascontiguousarray(x0[:, None]), 4, un.FZ_REL, 0.0, ter, dist, None)
    ok = ~un.near_samples("episode after reset", ref)[:, 0]
    for f in tc.INTS_T:
        assert np.array_equal(t_a[f][ok], ref["trows"][f][ok, 0]), f
    epi.close(); A.close()
