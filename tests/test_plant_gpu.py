"""The per-sample plant (include/hsddp_plant.h; the ten kernels of cafe-mpc_amd/csrc/hsddp_plant.hip) on the device: a nominal table against the plant
off, the cases of tests/plant_common.py against the restated reference walks with the device's own policy, isolation of the samples, the prefix
property, refusals and allocation, and episodes with a plant per robot and the pending reset map on the robot's own links."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import sim_common as sc
import mc_common as mc
import uni_common as un
import ter_common as tc
import plant_common as pc

pytestmark = pytest.mark.gpu

EINVAL = -1
MU = 0.6
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
Dist = pkg.sim.Disturbance
Plant = pkg.sim.Plant
ep = pkg.episode
INTS_C = ("first_release", "n_release", "n_land", "n_free", "free_final")


@pytest.fixture(scope="module")
def trot12(oracle_lib, hip_lib):
    """trot12 of tests/test_terrain_gpu.py: trot 4 x 12, B = 4, 3 AL x 4 DDP, R = 8 samples around Xbar[0]; the policy rows of the DEVICE handle."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    sg = pkg.MultiPhaseDDP(phases, batch=4)
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); sg.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(sg.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, sg, xs, mc.policy_of(sg)
    sg.close()


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return pc.build_ref(pkg, tmp_path_factory.mktemp("plant_ref_gpu"))


def same_bits(a, b):
    assert set(a) == set(b)
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("family,case,S", [("bi", "plain", 1), ("bi", "plain", 3), ("uni", "flight", 4), ("ter", "block", 4)])
def test_nominal_table_is_the_plant_off_run(trot12, family, case, S):
    """Case 1: a one-row nominal table (the _plant kernels) against the plant off (today's kernels): integer rows equal, floats within the tolerance.
    Every added operation is exact at nominal (x 1, + 0, - 0 qdot), so bit-identity is expected: printed, not asserted."""
    phases, sg, xs, pol = trot12
    x0, d, k, fz_rel, zg, ter, _ = pc.case_of(pkg, family, case, S, "mixed", xs)
    res = pc.library_run(pkg, sg, x0, 48, S, Plant.nominal(), family, fz_rel, zg, ter, d, k, MU)
    base = pc.library_run(pkg, sg, x0, 48, S, None, family, fz_rel, zg, ter, d, k, MU)
    assert set(res) == set(base)
    print(f"[plant] gpu nominal {family} {case} S={S}: bit-identical to the plant off: {all(res[f].tobytes() == base[f].tobytes() for f in base)}")
    assert np.array_equal(res["rows"]["first_bad"], base["rows"]["first_bad"]) and (base["rows"]["first_bad"] < 0).all()
    assert np.array_equal(res["grf"]["n_slip"], base["grf"]["n_slip"]) and np.array_equal(res["grf"]["first_slip"], base["grf"]["first_slip"])
    if "extra" in base:
        assert np.array_equal(res["extra"], base["extra"])
    if "contact" in base:
        assert base["contact"]["n_release"].sum() > 0
        for f in INTS_C:
            assert np.array_equal(res["contact"][f], base["contact"][f]), f
        sc.close("max_lift", res["contact"]["max_lift"], base["contact"]["max_lift"], scale=1.0)
    if "terrain" in base:
        assert base["terrain"]["n_early"].sum() > 0
        for f in tc.INTS_T:
            assert np.array_equal(res["terrain"][f], base["terrain"][f]), f
        sc.close("max_pen", res["terrain"]["max_pen"], base["terrain"]["max_pen"], scale=1.0)
    for f in ("X", "U", "x_final", "Y"):
        sc.close(f"gpu nominal {f}", res[f], base[f], scale=max(1.0, float(np.abs(base[f]).max())))
    for f in ("dev_q", "dev_v", "min_height", "max_torque"):
        sc.close(f"gpu nominal {f}", res["rows"][f], base["rows"][f], scale=max(1.0, float(np.abs(base["rows"][f]).max())))
    for f in ("min_fz", "min_cone", "max_fz"):
        fin = np.isfinite(base["grf"][f])
        assert np.array_equal(np.isfinite(res["grf"][f]), fin)
        sc.close(f"gpu nominal {f}", res["grf"][f][fin], base["grf"][f][fin], scale=max(1.0, float(np.abs(base["Y"]).max())))


@pytest.mark.parametrize("family,case,S,table", pc.CASES)
def test_plant_cases_match_the_reference(trot12, ref_lib, family, case, S, table):
    """Case 2, the cases of plant_common.CASES (tests/test_plant_host.py has their margins): non-vacuity first, on the references alone - every sample
    of a non-nominal row moves by more than 1e-3 in X against the reference at nominal - and the cap of one left-out sample, then the run against the
    restated reference walk under the project's tolerances."""
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, pl = pc.case_of(pkg, family, case, S, table, xs)
    B = x0.shape[0]
    if B == 4:
        s, polB = sg, pol
    else:      # fewer problems: a handle of that batch with the same problems, its own policy rows
        s = pkg.MultiPhaseDDP(phases, batch=B)
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)[:B]); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
        polB = mc.policy_of(s)
    ref = pc.reference_of(pkg, ref_lib, phases, polB, smap, family, x0, S, fz_rel, zg, ter, pl, d, k)
    nominal = pc.reference_of(pkg, ref_lib, phases, polB, smap, family, x0, S, fz_rel, zg, ter, Plant.nominal(), d, k)
    live = (ref["first_bad"] < 0) & (nominal["first_bad"] < 0)
    pc.assert_table_moves_the_reference(f"gpu {case} S={S}", {"X": ref["X"][live][None]}, {"X": nominal["X"][live][None]}, Plant(pl.rows, plant_of=np.asarray(pl.plant_of)[live][None]))
    res = pc.library_run(pkg, s, x0, 48, S, pl, family, fz_rel, zg, ter, d, k, MU)
    contact = np.array([[phases[int(p)]["desc"].contact[l] for l in range(4)] for p in smap[0]])
    pc.compare(pkg, f"gpu {case} S={S}", family, res, ref, mc.xbar_window(polB, smap), contact, MU, fz_rel)
    if case == "divergence":
        assert res["rows"]["first_bad"][1, 1] == 5 and np.array_equal(res["X"][1, 1, 6:], np.broadcast_to(res["x_final"][1, 1], (43, 36)))
    if s is not sg:
        s.close()


def collect(sim, disturbed, contact=False, terrain=False):
    rows, xf = sim.rows(); X, U = sim.traj()
    out = dict(rows=rows, x_final=xf, X=X, U=U)
    if disturbed:
        out["extra"] = sim.extra()
    if contact:
        out["contact"] = sim.contact_rows()
    if terrain:
        out["terrain"] = sim.terrain_rows()
    return out


def test_samples_are_isolated_and_the_plant_toggles(trot12):
    """Case 3 on the block case, S = 4: the samples of a nominal row are bit-identical to a run with a one-row nominal table; permuting the rows and
    re-indexing plant_of changes no bit; a run after clear_plant is bit-identical to one before set_plant, and so is the bilateral walk at S = 1 and
    with the records off (the kernels without records and sub-step loop again)."""
    phases, sg, xs, pol = trot12
    x0, d, k, fz_rel, zg, ter, pl = pc.case_of(pkg, "ter", "block", 4, "mixed2", xs)
    res = pc.library_run(pkg, sg, x0, 48, 4, pl, "ter", fz_rel, zg, ter, d, k, MU)
    alone = pc.library_run(pkg, sg, x0, 48, 4, Plant.nominal(), "ter", fz_rel, zg, ter, d, k, MU)
    n0 = np.asarray(pl.plant_of) == 0
    for f in res:
        assert res[f][n0].tobytes() == alone[f][n0].tobytes(), f
    assert not np.array_equal(res["x_final"][~n0], alone["x_final"][~n0])
    perm = np.array([2, 0, 1]); inv = np.argsort(perm)
    same_bits(pc.library_run(pkg, sg, x0, 48, 4, Plant(pl.rows[perm], plant_of=inv[np.asarray(pl.plant_of)].astype(np.int32)), "ter", fz_rel, zg, ter, d, k, MU), res)
    sim = pkg.Simulation(sg, 8, 48, keep_traj=True)
    try:      # (a simulation object must not outlive its handle: closed whatever an assertion says)
        toggles(sim, xs, x0, d, k, fz_rel, zg, ter, pl, res, n0)
    finally:
        sim.close()


def toggles(sim, xs, x0, d, k, fz_rel, zg, ter, pl, res, n0):
    assert sim.plant[0] is False and sim.plant[1].shape == (0, 46)
    sim.run(xs); plain1 = collect(sim, False)                                   # k_sim_quad
    sim.set_substeps(4); sim.set_contact(fz_rel, zg); sim.set_terrain(ter)
    sim.run(x0, dist=d, kick=k); before = collect(sim, True, True, True)
    sim.set_plant(pl)
    on, rows = sim.plant
    assert on and np.array_equal(rows, pl.table())
    sim.run(x0, dist=d, kick=k); with_plant = collect(sim, True, True, True)
    for f in ("rows", "x_final", "X", "U", "extra", "contact", "terrain"):
        assert with_plant[f].tobytes() == res[f].tobytes(), f                   # the object path is the one-off path
    sim.clear_plant(); assert sim.plant[0] is False and np.array_equal(sim.plant[1], pl.table())
    sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, True, True), before)
    sim.clear_contact(); sim.set_substeps(1); sim.set_plant(pl)
    sim.run(xs); bi = collect(sim, False)
    assert np.abs(bi["X"][~n0] - plain1["X"][~n0]).max() > 1e-3      # k_sim_quad_plant: the samples of a payload row move, those of the nominal row
    sc.close("bilateral nominal rows", bi["X"][n0], plain1["X"][n0])      # are k_sim_quad's within the tolerance (another kernel: not bit for bit)
    sim.clear_plant(); sim.run(xs); same_bits(collect(sim, False), plain1)


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_plant_contract(trot12, hip_lib):
    """Case 4: the first 24 steps of a 48-step run equal a 24-step run; every refusal of the header is returned with nothing changed; runs do not
    allocate, a set call only when it is the first or the table grows; the handle is left bit for bit as it was."""
    phases, sg, xs, pol = trot12
    x0, d, k, fz_rel, zg, ter, pl = pc.case_of(pkg, "ter", "block", 4, "mixed2", xs)
    d16 = dataclasses.replace(d, kick_step=16)      # inside both windows
    long = pc.library_run(pkg, sg, x0, 48, 4, pl, "ter", fz_rel, zg, ter, d16, k, MU)
    short = pc.library_run(pkg, sg, x0, 24, 4, pl, "ter", fz_rel, zg, ter, d16, k, MU)
    assert np.array_equal(long["X"][:, :, :24], short["X"][:, :, :24]) and np.array_equal(long["U"][:, :, :24], short["U"]) and np.array_equal(long["Y"][:, :, :24], short["Y"])
    assert np.array_equal(long["X"][:, :, 24, :18], short["X"][:, :, 24, :18])      # (entry 24 of the long run lies behind a reset map: positions stay)
    lib = pkg._abi.bind_plant(hip_lib)
    phases6 = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases6, batch=4); s.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    x2 = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 2, 0.02, 0.2, seed=4)
    snap = snapshot(s)
    sim = pkg.Simulation(s, 2, 20, keep_traj=True)
    try:
        contract(sim, s, x2, snap, lib, hip_lib)
    finally:
        sim.close(); s.close()


def contract(sim, s, x2, snap, lib, hip_lib):
    sim.run(x2); first = collect(sim, False)
    P, po, bad = pc.bad_tables(pkg)
    vp = lambda a: None if a is None else a.ctypes.data
    setp = lambda n, rows, of, on=1: lib.hsddp_plant_set(sim.s, on, n, vp(rows), vp(of))
    on, n = ctypes.c_int(-7), ctypes.c_int(-7)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_plant_get_params(sim.s, ctypes.byref(on), ctypes.byref(n)) == 0 and (on.value, n.value) == (0, 0)
    assert lib.hsddp_plant_set(None, 1, 3, vp(P), vp(po)) == EINVAL and lib.hsddp_plant_set(None, 0, 0, None, None) == EINVAL
    assert setp(0, P, po) == EINVAL and setp(-1, P, po) == EINVAL and setp(65537, P, None) == EINVAL and setp(2, P, po) == EINVAL
    for rows, of in bad:
        assert setp(3, rows, of) == EINVAL
    out = np.zeros((3, 46))
    assert lib.hsddp_plant_get_table(sim.s, 0, 1, out.ctypes.data) == EINVAL      # no table yet
    assert lib.hsddp_plant_get_params(None, ctypes.byref(on), ctypes.byref(n)) == EINVAL and lib.hsddp_plant_get_params(sim.s, None, ctypes.byref(n)) == EINVAL
    assert setp(0, None, None, on=0) == 0                                         # off on an object that never had it on: nothing to do
    assert hip_lib.hsddp_debug_malloc_count() == mallocs and sim.plant[0] is False
    sim.run(x2); same_bits(collect(sim, False), first)                            # the refused calls changed nothing
    good = Plant(pc.three_rows(pkg), plant_of=po.reshape(4, 2))
    sim.set_plant(good)
    assert hip_lib.hsddp_debug_malloc_count() > mallocs                           # the first on allocates
    for rows, of in bad[:3] + bad[-1:]:
        assert setp(3, rows, of) == EINVAL
    assert sim.plant[0] and np.array_equal(sim.plant[1], good.table())            # a refused call leaves the table
    assert lib.hsddp_plant_get_table(sim.s, 1, 2, out.ctypes.data) == 0 and np.array_equal(out[:2], good.table()[1:])
    assert lib.hsddp_plant_get_table(sim.s, 2, 2, out.ctypes.data) == EINVAL and lib.hsddp_plant_get_table(sim.s, -1, 1, out.ctypes.data) == EINVAL
    assert lib.hsddp_plant_get_table(sim.s, 0, 3, None) == EINVAL and lib.hsddp_plant_get_table(None, 0, 1, out.ctypes.data) == EINVAL
    sim.run(x2); one = collect(sim, False)
    assert not np.array_equal(one["X"], first["X"])
    sim.run(x2, dist=Dist(seed=3, u_max=17.0)); sim.run(x2, dist=Dist(seed=3, sigma_u=0.1)); sim.set_grf(MU); sim.run(x2); sim.set_substeps(3); sim.run(x2)      # first uses of the others
    sim.set_contact(-3.0, 0.0); sim.run(x2); sim.set_terrain(pkg.sim.Terrain(H=np.zeros((1, 2, 2)), cx=0.5, cy=0.5, early=True, w_td=0.05)); sim.run(x2)
    m2 = hip_lib.hsddp_debug_malloc_count()
    sim.set_plant(Plant.nominal(2)); sim.run(x2)                                  # a smaller table: the block that is there holds it
    sim.clear_plant(); sim.run(x2); sim.set_plant(good); sim.run(x2); sim.run(x2, dist=Dist(seed=3, sigma_u=0.1)); sim.clear_terrain(); sim.run(x2); sim.run(x2, dist=Dist(seed=3, u_max=17.0))
    sim.clear_contact(); sim.set_substeps(1); sim.set_grf(0.0); sim.run(x2)
    again = collect(sim, False)
    assert hip_lib.hsddp_debug_malloc_count() == m2                               # no run allocates, nor a set call whose table fits
    same_bits(again, one)
    sim.set_plant(Plant.nominal(4)); assert hip_lib.hsddp_debug_malloc_count() == m2 + 1      # the table grows: one block
    sim.run(x2); assert hip_lib.hsddp_debug_malloc_count() == m2 + 1
    after = snapshot(s)
    for kf in snap:
        assert snap[kf].tobytes() == after[kf].tobytes(), kf                      # the handle is bit for bit what it was
    # (HSDDP_ENOTSUP needs an fp32 handle, which cannot hold the whole-body knots a simulation object asks for: not reachable here)


def test_three_tick_episode_with_a_plant_per_robot(request, trot12, hip_lib, ref_lib):
    """Case 5: ter_common.episode_phases, B = 4, n_exec = 12, three ticks with hsddp_reconfigure and a solve between them, S = 4, torque limit, the
    contact rule and the episode's block terrain, a plant per robot (nominal, 1 kg, 2 kg with scaled links, 1 kg).  A tick of 12 steps ends ON a
    touchdown, so every tick is followed by the pending reset map on the robot's own links (k_episode_impact_plant; n_impacts asserted).  Every tick is
    compared with the restated reference walked from the episode's state before the tick, with the policy read from the handle and the REFERENCE's
    (F, E) handed from tick to tick, and the reference's impact with the robot's links behind it.  The table survives reconfigure and reset.  With the
    plant switched off again the episode is bit-identical to one that never had a plant."""
    B, T, n = 4, 3, 12
    phases = tc.episode_phases(pkg)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241222)
    opt0, opt_rt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4), pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    ter = tc.terrain_of(pkg, "episode", (B, 1))
    pl = Plant(pc.three_rows(pkg), plant_of=np.array([0, 1, 2, 1], dtype=np.int32))
    dist = Dist(seed=mc.SEED, u_max=8.0, kick_step=0)
    kick = np.zeros((B, 36))
    ident = (list(range(len(phases))), [0] * len(phases))
    smap = sc.step_map(phases, n)
    D = [p["desc"] for p in phases]

    def episode(A, plant, clear=False):
        e = A.episode(n, T, keep_log=True); e.set_grf(MU); e.set_substeps(4); e.set_contact(un.FZ_REL, 0.0); e.set_terrain(ter)
        if plant is not None:
            e.set_plant(plant)
        if clear:
            e.set_plant(None, on=False)
        return e
    A = pkg.MultiPhaseDDP(phases, batch=B); request.addfinalizer(A.close)      # (finalizers run last in, first out: an episode never outlives its handle)
    epi = episode(A, pl); request.addfinalizer(epi.close)
    epi.reset(x0); A.solve(opt0)
    state, F, E = x0.copy(), np.zeros((B, 1, 4), dtype=bool), np.zeros((B, 1, 4), dtype=bool)
    moved = 0.0
    for t in range(T):
        pol = mc.policy_of(A)
        args = (phases, pol, smap, np.ascontiguousarray(state[:, None]), 4, un.FZ_REL, 0.0, ter)
        dt_ = dataclasses.replace(dist, seed=ep.tick_seed(dist.seed, t))
        ref = pc.oracle_walk_ter_plant(pkg, ref_lib, *args, Plant(pl.rows, plant_of=np.asarray(pl.plant_of)[:, None]), dt_, None, F0=F, E0=E)
        nominal = pc.oracle_walk_ter_plant(pkg, ref_lib, *args, Plant.nominal(), dt_, None, F0=F, E0=E)
        live0 = epi.rows()[0]["end_reason"] == 0
        epi.advance(dist, kick)
        erows, x_now = epi.rows(); c = epi.contact_rows(); tr = epi.terrain_rows()
        near = un.near_samples(f"plant episode tick {t}", ref)[:, 0]
        ok = live0 & ~near & (ref["first_bad"][:, 0] < 0)
        pi = int(smap[0, -1])
        want = np.stack([pc.impact_ref(pkg, ref_lib, D[pi], ref["X"][b, 0, -1], pl.table()[pl.plant_of[b]]) for b in range(B)])
        diff = np.abs(ref["X"][:, 0] - nominal["X"][:, 0]).max(axis=(-2, -1))
        moved = max(moved, float(diff[1:].min()))
        print(f"[plant] episode tick {t}: |X - X_nominal| per robot {diff}, free_final {c['free_final']}, early_final {tr['early_final']}, compared {int(ok.sum())} of {B}, "
              f"impact moves v by {np.abs(want - ref['X'][:, 0, -1]).max():.3e}")
        assert ok.sum() >= B - 1 and diff[0] == 0.0
        for f in INTS_C:
            assert np.array_equal(c[f][ok], ref["rows"][f][ok, 0]), (t, f, c[f], ref["rows"][f][:, 0])
        for f in tc.INTS_T:
            assert np.array_equal(tr[f][ok], ref["trows"][f][ok, 0]), (t, f, tr[f], ref["trows"][f][:, 0])
        sc.close(f"plant episode tick {t} state", x_now[ok], want[ok])
        assert np.abs(want - ref["X"][:, 0, -1]).max() > 1e-3      # the pending map did something
        state, F, E = x_now, ref["F"], ref["E"]
        A.reconfigure(phases, *ident); A.solve(opt_rt)
    assert moved > 1e-3 and epi.status()[2] == T      # every tick ended on a touchdown: three pending maps
    epi.reset(x0)                                     # the table survives a reset (and survived the reconfigures above)
    on, n_pl = ctypes.c_int(), ctypes.c_int()
    assert pkg._abi.bind_plant(hip_lib).hsddp_plant_get_params(hip_lib.hsddp_episode_sim(epi.e), ctypes.byref(on), ctypes.byref(n_pl)) == 0 and (on.value, n_pl.value) == (1, 3)
    epi.close(); A.close()
    # dormancy: set and switched off again against never set, same solver sequence
    logs = []
    for clear in (False, True):
        A = pkg.MultiPhaseDDP(phases, batch=B); request.addfinalizer(A.close)
        e = episode(A, pl if clear else None, clear=clear); request.addfinalizer(e.close)
        e.reset(x0); A.solve(opt0)
        for t in range(2):
            e.advance(dist, kick); A.reconfigure(phases, *ident); A.solve(opt_rt)
        logs.append((e.rows()[0].tobytes(), e.rows()[1].tobytes()) + tuple(a.tobytes() for a in e.log()))
        e.close(); A.close()
    assert logs[0] == logs[1]
