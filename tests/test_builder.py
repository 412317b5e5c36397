"""Host-side problem builder (cafe_mpc_amd.builder): MHPCProblem::initialization + QuadReference restated, driven by the gait
files and settings the reference ships (trimmed copies under tests/golden/cafe_tree, made by tests/golden/make_gait_fixture.py)."""
import importlib
import os

import numpy as np
import pytest

from conftest import pkg, ROOT
import parity_common as pc

builder = importlib.import_module(pkg.__name__ + ".builder")
TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")


def test_quad_reference_loader_semantics():
    ref = builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"))
    assert len(ref) == 130 and ref.dt == np.float32(0.01)
    # std::stof parsing: values are float32 numbers widened to double (QuadReference.cpp:170-332)
    bs = ref.tp["body_state"]
    assert np.array_equal(bs, bs.astype(np.float32).astype(np.float64))
    # reorder_body_states: file order [eul, pos, omega, vWorld] -> [pos, eul, vWorld, omega]; the file's 6th number is the body height
    assert abs(bs[0, 2] - np.float32(0.146)) < 1e-12 or bs[0, 2] > 0.1
    ref.initialize(0.75)
    assert ref.sz == 76
    # nearest-sample lookup in float arithmetic (QuadReference.cpp:63-76)
    assert ref.index(0.0) == 0 and ref.index(0.014) == 1 and ref.index(0.016) == 2 and ref.index(10.0) == 75
    swapped = builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True)
    assert np.array_equal(swapped.tp["contact"], ref.tp["contact"][:, [1, 0, 3, 2]]) and not swapped.tp["jnt_vel"].any()


def test_mhpc_problem_from_shipped_bound_gait():
    phases, info, cfg = builder.build_from_tree(TREE)         # mhpc_config.info: bound, 0.25 s whole-body + 0.5 s SRB
    assert cfg["referenceFile"] == "bound" and info["horizons"] == [6, 10, 9] and info["srb_horizon"] == 10
    assert info["contacts"] == [[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]]
    d = [p["desc"] for p in phases]
    assert [x.model for x in d] == [0, 0, 0, 1] and [x.next_model for x in d][:3] == [0, 0, 1]
    assert list(d[2].next_contact) == [0, 0, 1, 1]             # hind feet land 0.27 s into the plan: touchdown constraint + impact + projection
    assert abs(d[0].reb_torque.delta - 1.0) < 1e-15 and abs(d[0].reb_grf.eps - 0.05) < 1e-15 and d[0].al_td.sigma == 20.0
    assert list(d[0].q)[:6] == [0, 0, 10, 1, 2, 2] and abs(d[3].r[0] - 0.01) < 1e-15 and d[3].dt == 0.05
    assert np.allclose(phases[0]["bufs"]["yr"][0], [0, 0, 22.5] * 4)       # GRF reference of the first sample
    # the trimmed fixture reproduces what the full tree gives (stored by tests/golden/make_gait_fixture.py)
    full = np.load(os.path.join(ROOT, "tests", "golden", "full_tree_bound_bufs.npz"))
    assert list(full["horizons"]) == info["horizons"]
    assert len(full.files) == 1 + sum(len(p["bufs"]) for p in phases)
    for i, a in enumerate(phases):
        for k in a["bufs"]:
            assert np.array_equal(a["bufs"][k], full[f"p{i}_{k}"]), (i, k)


@pytest.mark.parametrize("gait", ["bound", "trot/dynfeas"])
def test_oracle_solves_shipped_gaits(oracle_lib, gait):
    phases, info, cfg = builder.build_from_tree(TREE, gait=gait, ubar_mode="gravity_comp")
    opt = builder.load_ddp_setting(os.path.join(TREE, "MHPC/settings/ddp_setting.info"))
    s = pkg.Solver(oracle_lib, phases, batch=1)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(info["x0"][None])
    s.hybrid_rollout(0.0, opt); s.compute_cost(opt)
    f0 = s.measure_dynamics_feasibility()[0]
    s.solve(opt)
    ia = s.info_arrays()
    assert ia["status"][0] == 0 and ia["n_iters"][0] >= 2
    assert ia["dyn_feas"][0] < 0.2 * f0 and ia["max_tconstr"][0] < 5e-3


def test_hkd_problem_from_shipped_bound_gait(oracle_lib):
    """HKDProblem::initialization + HKDMPCSolver constants on the gait file HKDMPC.h:30 names, solved by the oracle; foot-placement
    extraction (HKDMPC.cpp:207-240) returns the landing spots the reset map projected on the ground."""
    ref = builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True)
    cpar = builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info"))
    phases, info = builder.build_hkd_problem(ref, cpar)
    assert sum(info["horizons"]) == 60 and info["contacts"][0] == [1, 1, 1, 1] and info["contacts"][1] == [1, 1, 0, 0]      # FR FL HR HL: front stance
    d0 = phases[0]["desc"]
    assert d0.model == pkg.MODEL_HKD and abs(d0.reb_grf.eps - 0.5) < 1e-15 and d0.al_td.sigma == 20.0 and abs(d0.mu - 0.7) < 1e-15
    opt = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info"))
    s = pkg.Solver(oracle_lib, phases, batch=1)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(info["x0"][None])
    s.hybrid_rollout(0.0, opt); s.compute_cost(opt); f0 = s.measure_dynamics_feasibility()[0]
    s.solve(opt)
    ia = s.info_arrays()
    # cold start on a kinematic (not dynamically consistent) reference with 5 x 10 iterations: the defects close, the plan is not converged
    assert ia["status"][0] == 0 and ia["n_iters"][0] == 50 and ia["dyn_feas"][0] < 0.2 * f0
    pf = builder.hkd_next_footholds(s, info["contacts"])
    assert set(pf) >= {2, 3} and all(abs(v[2]) < 1e-12 for v in pf.values())       # hind legs land first; cmap = (1,1,0) puts the foothold on z = 0


def _fnv(chunks):
    h = 1469598103934665603
    for c in chunks:
        for byte in c:
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("gait", ["bound", "trot/dynfeas"])
def test_cpp_builder_matches_python_mirror(tmp_path, gait):
    """cafe-mpc_amd/host/mhpc_builder.hpp (what a CAFE-MPC maintainer links) and cafe_mpc_amd.builder produce identical descriptors —
    phase table, flags, every reference array and weight, bit for bit — at initialisation and over 12 receding-horizon updates."""
    import json, subprocess
    exe = tmp_path / "builder_dump"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "builder_dump.cpp"), "-o", str(exe)])
    nticks = 12
    cpp = json.loads(subprocess.check_output([str(exe), TREE, gait, str(nticks)]))
    cfg = builder.load_mhpc_config(TREE + "/MHPC/settings/mhpc_config.info")
    pd = builder.MHPCProblemData(builder.QuadReference(os.path.join(TREE, "Reference/Data", gait, "quad_reference.csv")), cfg,
                                 builder.load_cost_weights(TREE + "/" + cfg["costFile"]), builder.load_constraint_params(TREE + "/" + cfg["constraintParamFile"]))
    for tick in range(nticks + 1):
        if tick:
            pd.update()
        phases, _ = pd.describe()
        assert len(phases) == len(cpp[tick])
        for p, c in zip(phases, cpp[tick]):
            d, B = p["desc"], p["bufs"]
            assert (d.model, d.horizon, d.shooting, d.c_touchdown, d.next_model) == (c["model"], c["h"], c["shooting"], c["c_touchdown"], c["next_model"])
            assert list(d.contact) == c["contact"] and list(d.next_contact) == c["next_contact"] and d.w_td_vel == c["w_td_vel"]
            assert abs(d.t_offset - c["t_offset"]) < 1e-6 and abs(d.dt - c["dt"]) < 1e-12
            arrays = [B["xr"], B["ur"]] + ([B["yr"]] if "yr" in B else [np.zeros(0)]) + [B["foot_pos"], B["foot_vel"], B["body_pos"], B["ref_contact"], p["Xbar"]]
            assert str(_fnv(np.ascontiguousarray(a).tobytes() for a in arrays)) == c["hash"], (tick, d.model, d.horizon)
            import ctypes
            wb = [bytes(d.q), bytes(d.r), bytes(d.qf), ctypes.string_at(ctypes.addressof(d.reb_torque), 4 * ctypes.sizeof(d.reb_torque)), bytes(d.al_td)]
            assert str(_fnv(wb)) == c["whash"]


def test_hkd_receding_horizon_update_rules(oracle_lib, tmp_path):
    """HKDProblem::update (HKDMPC/HKD-TrajOpt/HKDProblem.cpp:117-222) over 30 MPC ticks of the shipped bound gait: the window keeps its 60 knots, a
    contact change at the horizon end first grows the last phase and then appends a young phase that has no shooting nodes until it is longer
    than two knots (:211-216), touchdown constraints appear when a phase's end has been seen (:201-204), no phase gets the constraint twice on
    this gait.  The C++ builder (host/mhpc_builder.hpp HkdProblemData) emits the same descriptors bit for bit.  The MPC loop of
    HKDMPC.cpp:97-143 (2 AL x 1 DDP per tick, window moved inside the handle, first control zeroed) runs on the oracle."""
    import json, subprocess, ctypes
    exe = tmp_path / "builder_dump"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "builder_dump.cpp"), "-o", str(exe)])
    nticks = 30
    cpp = json.loads(subprocess.check_output([str(exe), TREE, "bound", str(nticks), "hkd"]))
    ref = builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True)
    pd = builder.HKDProblemData(ref, builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info")))
    young = 0
    for tick in range(nticks + 1):
        if tick:
            m = pd.update()
            assert all(v[0] in (0, 1, 2) and v[1] in (0, 1, 2) for v in m.values())
        phases, info = pd.describe()
        assert sum(info["horizons"]) == 60 and len(phases) == len(cpp[tick])
        assert all(s == 1 for s in info["shooting"][:-1]) and (info["shooting"][-1] == 1) == (info["horizons"][-1] > 2 or tick == 0)
        young += info["shooting"][-1] == 0
        for p, c in zip(phases, cpp[tick]):
            d, B = p["desc"], p["bufs"]
            assert (d.model, d.horizon, d.shooting, d.c_touchdown, d.next_model) == (c["model"], c["h"], c["shooting"], c["c_touchdown"], c["next_model"])
            assert list(d.contact) == c["contact"] and list(d.next_contact) == c["next_contact"] and abs(d.t_offset - c["t_offset"]) < 1e-6
            arrays = [B["xr"], B["ur"], np.zeros(0), B["foot_pos"], B["foot_vel"], B["body_pos"], B["ref_contact"], p["Xbar"]]
            assert str(_fnv(np.ascontiguousarray(a).tobytes() for a in arrays)) == c["hash"], (tick, d.horizon)
            wb = [bytes(d.q), bytes(d.r), bytes(d.qf), ctypes.string_at(ctypes.addressof(d.reb_torque), 4 * ctypes.sizeof(d.reb_torque)), bytes(d.al_td)]
            assert str(_fnv(wb)) == c["whash"]
    assert young >= 5 and pd.dup_td == 0
    # the loop on the oracle
    ref = builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True)
    pd = builder.HKDProblemData(ref, builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info")))
    opt0 = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info")); opt0.max_AL_iter, opt0.max_DDP_iter = 2, 4
    opt_rt = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info")); opt_rt.max_AL_iter, opt_rt.max_DDP_iter = 2, 1      # HKDMPC.cpp:102-103
    phases, info = pd.describe()
    s = pc.make_pair(pkg, oracle_lib, oracle_lib, phases, info["x0"][None])[0]
    s.solve(opt0)
    for tick in range(1, 7):
        m = pd.update(); old = phases
        phases, inf = builder.shift_solver_in_place(s, old, pd, m)
        assert np.abs(s.field(0, "UBAR")[:, 0]).max() > 0
        s.set_control_knot(0, 0, None)
        assert np.abs(s.field(0, "UBAR")[:, 0]).max() == 0 and np.abs(s.field(0, "UBAR")[:, 1]).max() > 0
        s.set_initial_condition(np.ascontiguousarray(s.field(0, "XBAR")[:, 0])); s.solve(opt_rt)
        ia = s.info_arrays()
        assert ia["status"][0] == 0 and ia["n_iters"][0] == 2 and np.isfinite(ia["actual_cost"][0])
        si = s.export_solver_info(0)
        assert (si["n_iter"], si["n_ls_iter"]) == (ia["n_iters"][0], ia["n_ls_iters"][0]) and si["cost"] == np.float32(ia["actual_cost"][0]) and si["eq_violation"] == np.float32(ia["max_tconstr"][0])


def _mpc_setup():
    cfg = builder.load_mhpc_config(TREE + "/MHPC/settings/mhpc_config.info")
    pd = builder.MHPCProblemData(builder.QuadReference(TREE + "/Reference/Data/bound/quad_reference.csv"), cfg,
                                 builder.load_cost_weights(TREE + "/" + cfg["costFile"]), builder.load_constraint_params(TREE + "/" + cfg["constraintParamFile"]))
    opt0 = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info")
    opt_rt = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info")
    opt_rt.max_AL_iter, opt_rt.max_DDP_iter = opt_rt.max_AL_iter_runtime, opt_rt.max_DDP_iter_runtime       # MHPCLocomotion.cpp:113-115
    return cfg, pd, opt0, opt_rt


def test_constraint_parameters_survive_the_receding_horizon_shift(oracle_lib):
    """The reference's phase objects keep their constraint parameters across MPC ticks: per-knot ReB parameters are popped / pushed with
    their knots (a pushed knot copies the last knot's, ConstraintsBase.h:296-306, reset_params() is a no-op :192), AL parameters stay
    with the phase.  The first solve (up to 20 AL iterations of update_params) changes them; the shifted window must start from the
    UPDATED values, whichever of the two ABI routes moves it (new handle + hsddp_warm_start_phase, or hsddp_reconfigure in place)."""
    cfg, pd, opt0, opt_rt = _mpc_setup()
    phases, info = pd.describe(ubar_mode="gravity_comp")
    x0 = info["x0"][None]
    s = pc.make_pair(pkg, oracle_lib, oracle_lib, phases, x0)[0]
    s2 = pc.make_pair(pkg, oracle_lib, oracle_lib, phases, x0)[0]
    s.solve(opt0); s2.solve(opt0)
    eps0 = [s.field(i, "REB_EPS") for i in range(len(phases))]
    init = [p["desc"].reb_torque.eps for p in phases]
    changed = any(e.size and not np.allclose(e, e.flat[0]) for e in eps0) or any(s.field(i, "AL_SIGMA").size and (s.field(i, "AL_SIGMA") != phases[i]["desc"].al_td.sigma).any() for i in range(len(phases)))
    assert changed, "the first solve must have updated ReB or AL parameters for this test to mean anything"
    m = pd.update()
    nst = int(round(float(cfg["dt_mpc"]) / cfg["dt_wb"]))
    x0n = s.field(0, "XBAR")[:, nst]
    old_phases = phases
    sa, pha, infa = builder.shift_solver(pkg.Solver, oracle_lib, s, old_phases, pd, m)          # route 1: new handle
    phb, infb = builder.shift_solver_in_place(s2, old_phases, pd, m)                              # route 2: in place
    uid_old = {p.get("uid"): i for i, p in enumerate(old_phases)}
    for i, p in enumerate(pha):
        for f in ("REB_EPS", "REB_DELTA", "AL_SIGMA", "AL_LAMBDA", "XBAR", "UBAR", "K"):
            assert np.array_equal(sa.field(i, f), s2.field(i, f)), (i, f)
        j = uid_old.get(p.get("uid"))
        if j is not None and p.get("uid") != -1 and eps0[j].size:
            sh = m[p.get("uid")][0]
            got = sa.field(i, "REB_EPS")[0]; src = eps0[j][0]
            for k in range(got.shape[0]):
                assert np.array_equal(got[k], src[min(k + sh, src.shape[0] - 1)]), (i, k)
    for q in (sa, s2):
        q.set_initial_condition(np.ascontiguousarray(x0n)); q.solve(opt_rt)
    ia, ib = sa.info_arrays(), s2.info_arrays()
    for k in ("actual_cost", "dyn_feas", "n_iters", "n_ls_iters"):
        assert np.array_equal(ia[k], ib[k]), k
    # the handle that was reconfigured kept counting regularisation iterations (quirk xi); the new handle started from zero
    assert (ib["n_reg_iters"] >= ia["n_reg_iters"]).all()
