"""Disturbed closed-loop simulation (include/hsddp_mc.h, kernel k_sim_quad_mc of cafe-mpc_amd/csrc/wb_sim.hpp) on the device: parity with the
oracle walk of tests/mc_common.py fed with the GPU handle's own policy, the torque normals seen directly, the all-off run against hsddp_sim_run,
determinism / seeds / shards / extension, device-resident inputs, refusals, no allocation when warm, and contained divergence after a push."""
import ctypes

import numpy as np
import pytest

from conftest import pkg
import parity_common as pc
import sim_common as sc
import mc_common as mc

pytestmark = pytest.mark.gpu

EINVAL = -1
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
Dist = pkg.sim.Disturbance


@pytest.fixture(scope="module")
def trot12(hip_lib):
    """The fixture of tests/test_sim_gpu.py: trot 4 x 12, B = 4, 3 AL x 4 DDP, R = 8 samples (sigma 0.02 / 0.2) around Xbar[0]."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    sg = pkg.MultiPhaseDDP(phases, batch=4); sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222))
    sg.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(sg.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, sg, xs, mc.policy_of(sg)
    sg.close()


def same(a, b, fields=("x_final", "X", "U")):
    return all(np.array_equal(a[f], b[f]) for f in fields if f in a) and a["rows"].tobytes() == b["rows"].tobytes() and a["extra"].tobytes() == b["extra"].tobytes()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_mc_parity_trot_48(oracle_lib, trot12, name):
    """Cases A - D over the 48-step window (a lift-off and both touchdowns) against the oracle walk with the GPU handle's XBAR, UBAR, K."""
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    d, k = mc.cases(pkg, xs.shape[:2])[name]
    ref = mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs, d, k)
    res = sg.simulate(xs, 48, keep_traj=True, dist=d, kick=k)
    assert res["extra"].shape == (4, 8) and np.array_equal(res["X"][:, :, -1], res["x_final"])
    mc.compare_disturbed(f"gpu {name}", res, ref, mc.xbar_window(pol, smap))
    if name == "C":
        assert (res["extra"]["first_fall"] >= 0).sum() >= 9 and (res["extra"]["n_sat"] > 0).all()
    lean = sg.simulate(xs, 48, dist=d, kick=k)      # without trajectories: the same rows, extras and final states
    assert set(lean) == {"rows", "x_final", "extra"} and same(lean, res, fields=("x_final",))


def test_mc_parity_trot_200(oracle_lib, hip_lib):
    """Case E, the config-3 shape: 4 x 50 knots, B = 2, R = 4, the whole 200-step horizon with the switches of D."""
    phases = pkg.problems.wb_trot_problem()
    sg = pkg.MultiPhaseDDP(phases, batch=2); sg.set_initial_condition(pkg.problems.wb_ensemble_x0(2, 20241222))
    sg.solve(pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(sg.field(0, "XBAR")[:, 0], 4, 0.02, 0.2, seed=20241222)
    smap = sc.step_map(phases, 200)
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    pol = mc.policy_of(sg)
    ref = mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs, d, k)
    res = sg.simulate(xs, 200, keep_traj=True, dist=d, kick=k)
    mc.compare_disturbed("gpu E", res, ref, mc.xbar_window(pol, smap))
    lean = sg.simulate(xs, 200, dist=d, kick=k)
    assert same(lean, res, fields=("x_final",))
    sg.close()


def step0_torque_noise(sg, xs, res):
    """U[:, :, 0] - (Ubar + K (x0 - Xbar)) of knot 0."""
    ub, K, xb = sg.field(0, "UBAR")[:, 0], sg.field(0, "K")[:, 0], sg.field(0, "XBAR")[:, 0]
    return res["U"][:, :, 0] - (ub[:, None] + np.einsum("bij,brj->bri", K, xs - xb[:, None]))


def test_mc_torque_normals_seen_directly(trot12):
    """sigma_u = 0.2 alone: the noise of step 0 is 0.2 x mc_normals(...)[:12] to 1e-12, also on a shard (first_problem = 5)."""
    phases, sg, xs, pol = trot12
    for first in (0, 5):
        res = sg.simulate(xs, 8, keep_traj=True, dist=Dist(seed=mc.SEED, sigma_u=0.2, first_problem=first))
        want = 0.2 * np.array([[pkg.sim.mc_normals(mc.SEED, first + b, r, 0)[:12] for r in range(8)] for b in range(4)])
        err = np.abs(step0_torque_noise(sg, xs, res) - want).max()
        print(f"[mc] torque normals of step 0, first_problem {first}: |diff| = {err:.3e}")
        assert err <= 1e-12
        assert np.array_equal(res["X"][:, :, 0], xs) and (res["extra"]["n_sat"] == 0).all() and (res["extra"]["first_fall"] == -1).all()


def test_mc_all_switches_off_is_the_plain_run(trot12):
    phases, sg, xs, pol = trot12
    sim = pkg.Simulation(sg, 8, 48, keep_traj=True)
    sim.run(xs); rows, xf = sim.rows(); X, U = sim.traj()
    with pytest.raises(RuntimeError):
        sim.extra()                                   # the last run was a plain one
    sim.run(xs, dist=Dist(seed=5, kick_step=99))      # (kick_step is read only with a kick)
    rows2, xf2 = sim.rows(); X2, U2 = sim.traj(); ex = sim.extra()
    assert rows.tobytes() == rows2.tobytes() and np.array_equal(xf, xf2) and np.array_equal(X, X2) and np.array_equal(U, U2)
    assert (ex["first_fall"] == -1).all() and (ex["n_sat"] == 0).all() and sim.kernel_time_ms() > 0.0
    sim.close()


def test_mc_determinism_seeds_shards_and_extension(oracle_lib, trot12):
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    a = sg.simulate(xs, 48, keep_traj=True, dist=d, kick=k)
    assert same(a, sg.simulate(xs, 48, keep_traj=True, dist=d, kick=k))                     # two runs: the same bytes
    other = Dist(**{**d.__dict__, "seed": d.seed + 1})
    assert not np.array_equal(a["U"], sg.simulate(xs, 48, keep_traj=True, dist=other, kick=k)["U"])      # another seed: other numbers
    # a shard: the same handle as problems 5..8 of a larger experiment (case A)
    dA, _ = mc.cases(pkg, xs.shape[:2])["A"]
    dA.first_problem = 5
    ref = mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs, dA)
    res = sg.simulate(xs, 48, keep_traj=True, dist=dA)
    mc.compare_disturbed("gpu A first_problem 5", res, ref, mc.xbar_window(pol, smap))
    dA0, _ = mc.cases(pkg, xs.shape[:2])["A"]
    assert not np.array_equal(res["U"], sg.simulate(xs, 48, keep_traj=True, dist=dA0)["U"])
    # more samples extend an experiment, a longer window extends a shorter one (case D)
    one = sg.simulate(np.ascontiguousarray(xs[:, :1]), 48, keep_traj=True, dist=d, kick=np.ascontiguousarray(k[:, :1]))
    for f in ("X", "U", "x_final"):
        assert np.array_equal(one[f][:, 0], a[f][:, 0]), f
    assert one["rows"][:, 0].tobytes() == a["rows"][:, 0].tobytes() and one["extra"][:, 0].tobytes() == a["extra"][:, 0].tobytes()
    short = sg.simulate(xs, 24, keep_traj=True, dist=d, kick=k)
    assert np.array_equal(short["X"][:, :, :24], a["X"][:, :, :24]) and np.array_equal(short["U"], a["U"][:, :, :24])


DEVICE_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")      # torch's runtime first, then the package's library
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package(); P = pkg.problems
phases = P.wb_trot_problem(horizons=(12, 12, 12, 12))
s = pkg.MultiPhaseDDP(phases, batch=4); s.set_initial_condition(P.wb_ensemble_x0(4, 20241222)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
xs = P.perturbed_states(s.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
kick = np.zeros((4, 8, 36)); kick[..., 19] = 0.3
d = pkg.sim.Disturbance(seed=20241222, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01, u_max=8.0, fall_height=0.16, kick_step=10)
out = {}
tx, tk = torch.from_numpy(xs).to("cuda"), torch.from_numpy(kick).to("cuda")
for kind, x, k in (("host", xs, kick), ("device", tx, tk), ("mixed", tx, kick)):
    r = s.simulate(x, 24, keep_traj=True, dist=d, kick=k)
    for f in ("X", "U", "x_final"):
        out[kind + "_" + f] = r[f]
    out[kind + "_rows"] = r["rows"].view(np.uint8); out[kind + "_extra"] = r["extra"].view(np.uint8)
for bad in (tk.float(), tk[:, :4], tk.cpu()):
    try:
        s.simulate(tx, 24, dist=d, kick=bad); raise SystemExit("accepted a bad kick tensor")
    except ValueError:
        pass
s.close()
np.savez(sys.argv[2], **out)
"""


def test_mc_device_tensors_give_the_same_bytes(trot12, tmp_path):
    """x0 and kick as torch device tensors against host arrays (in a process of its own: torch's HIP runtime has to be up first)."""
    import subprocess
    import sys
    from conftest import ROOT
    (tmp_path / "dev.py").write_text(DEVICE_SCRIPT)
    out = tmp_path / "out.npz"
    subprocess.check_call([sys.executable, str(tmp_path / "dev.py"), ROOT, str(out)], timeout=600)
    d = np.load(out)
    for kind in ("device", "mixed"):
        for k in ("X", "U", "x_final", "rows", "extra"):
            assert np.array_equal(d["host_" + k], d[kind + "_" + k]), (kind, k)
    phases, sg, xs, pol = trot12
    dd, k = mc.cases(pkg, xs.shape[:2])["D"]
    here = sg.simulate(xs, 24, keep_traj=True, dist=dd, kick=k)
    assert np.array_equal(d["host_X"], here["X"]) and d["host_extra"].tobytes() == here["extra"].tobytes()      # (and the same as in this process)


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_mc_leaves_the_handle_untouched(hip_lib):
    """The snapshot of test_sim_leaves_the_handle_untouched around a disturbed run, and a following solve against a twin that did not simulate."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    x0 = pkg.problems.wb_ensemble_x0(4, 20241222)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    a, b = [pkg.MultiPhaseDDP(phases, batch=4) for _ in range(2)]
    for s in (a, b):
        s.set_initial_condition(x0); s.solve(opt)
    before = snapshot(a)
    xs = pkg.problems.perturbed_states(a.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=3)
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    res = a.simulate(xs, 48, keep_traj=True, dist=d, kick=k)
    assert (res["rows"]["first_bad"] == -1).all() and np.abs(res["X"][:, :, 1:] - res["X"][:, :, :1]).max() > 1e-3
    after = snapshot(a)
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key
    for s in (a, b):
        s.solve(opt)
    sa, sb = snapshot(a), snapshot(b)
    for key in sa:
        assert sa[key].tobytes() == sb[key].tobytes(), key
    a.close(); b.close()


def test_mc_refusals_warm_runs_and_staleness(hip_lib):
    lib = pkg._abi.bind_mc(hip_lib)
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(pkg.problems.wb_ensemble_x0(5, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    kick = mc.kick_y((5, 3), 0.2)
    sim = pkg.Simulation(s, 3, 20, keep_traj=True)
    good = Dist(seed=1, sigma_u=0.1, sigma_q=0.001, sigma_v=0.01, u_max=10.0, fall_height=0.1, kick_step=4)
    run = lambda d, k=kick, x=xs, h=None: lib.hsddp_mc_run(sim.s if h is None else h, None if x is None else x.ctypes.data, 0, None if d is None else ctypes.byref(d.to_c()),
                                                          None if k is None else k.ctypes.data, 0)
    ex = np.zeros((5, 3), dtype=pkg._abi.MC_EXTRA_DTYPE)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    bad = [dict(sigma_u=-0.1), dict(sigma_q=-1e-3), dict(sigma_v=-1.0), dict(sigma_u=np.nan), dict(sigma_q=np.inf), dict(sigma_v=np.nan), dict(u_max=np.nan),
           dict(u_max=np.inf), dict(fall_height=np.nan), dict(fall_height=-np.inf), dict(first_problem=-1), dict(kick_step=-1), dict(kick_step=20)]
    for ch in bad:
        assert run(Dist(**{**good.__dict__, **ch})) == EINVAL, ch
    assert run(good, x=None) == EINVAL and run(None) == EINVAL and lib.hsddp_mc_run(None, xs.ctypes.data, 0, ctypes.byref(good.to_c()), None, 0) == EINVAL
    assert lib.hsddp_mc_get_extra(sim.s, 0, 5, ex.ctypes.data) == EINVAL                 # no run yet
    assert hip_lib.hsddp_debug_malloc_count() == mallocs                                  # nothing changed, nothing allocated
    assert run(Dist(**{**good.__dict__, "kick_step": 20}), k=None) == 0                     # without a kick the step is not read
    with pytest.raises(ValueError):
        sim.run(xs, dist=good, kick=kick[:, :1])
    sim.run(xs, dist=good, kick=kick); first = (sim.rows(), sim.extra(), sim.traj())
    mallocs = hip_lib.hsddp_debug_malloc_count()
    sim.run(xs, dist=good, kick=kick); second = (sim.rows(), sim.extra(), sim.traj())
    assert hip_lib.hsddp_debug_malloc_count() == mallocs                                  # a later disturbed run allocates nothing
    assert first[0][0].tobytes() == second[0][0].tobytes() and first[1].tobytes() == second[1].tobytes() and np.array_equal(first[2][0], second[2][0])
    assert sim.kernel_time_ms() > 0.0
    for b0, nb in ((-1, 1), (0, 0), (0, 6), (5, 1), (4, 2)):
        assert lib.hsddp_mc_get_extra(sim.s, b0, nb, ex.ctypes.data) == EINVAL, (b0, nb)
    assert lib.hsddp_mc_get_extra(sim.s, 0, 5, None) == EINVAL
    assert lib.hsddp_mc_get_extra(sim.s, 3, 2, ex.ctypes.data) == 0 and ex[:2].tobytes() == first[1][3:].tobytes()
    sim.run(xs)                                                                           # a plain run: its rows are served, the extras are refused
    assert lib.hsddp_mc_get_extra(sim.s, 0, 5, ex.ctypes.data) == EINVAL
    with pytest.raises(RuntimeError):
        sim.extra()
    assert (sim.rows()[0]["first_bad"] == -1).all()
    s.reconfigure(phases, list(range(len(phases))), [0] * len(phases))
    assert run(good) == EINVAL
    with pytest.raises(RuntimeError):
        sim.run(xs, dist=good, kick=kick)
    sim.close()
    sim2 = pkg.Simulation(s, 3, 20)                       # created again on the new window: runs, and gives the same numbers
    sim2.run(xs, dist=good, kick=kick)
    assert sim2.rows()[0].tobytes() == first[0][0].tobytes() and sim2.extra().tobytes() == first[1].tobytes()
    sim2.close(); s.close()


def test_mc_divergence_after_a_push_is_contained(trot12):
    """A kick of 1e7 on coordinate 18 of one sample: ordinary arithmetic on a large number.  The sample keeps the kicked state, reports
    first_bad = kick_step, and every other sample is bit-identical to the run without it."""
    phases, sg, xs, pol = trot12
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    clean = sg.simulate(xs, 48, keep_traj=True, dist=d, kick=k)
    k2 = k.copy(); k2[2, 5, 18] = 1e7
    res = sg.simulate(xs, 48, keep_traj=True, dist=d, kick=k2)
    assert res["rows"]["first_bad"][2, 5] == d.kick_step
    kicked = clean["X"][2, 5, d.kick_step] - k[2, 5] + k2[2, 5]
    assert np.array_equal(res["X"][2, 5, :d.kick_step], clean["X"][2, 5, :d.kick_step])
    assert np.allclose(res["x_final"][2, 5], kicked, rtol=0, atol=1e-8) and res["x_final"][2, 5, 18] > 9e6
    assert np.array_equal(res["X"][2, 5, d.kick_step:], np.repeat(res["x_final"][2, 5][None], 49 - d.kick_step, axis=0))
    assert res["extra"]["n_sat"][2, 5] <= clean["extra"]["n_sat"][2, 5] + 12      # only the step of the kick may still count
    keep = np.ones((4, 8), dtype=bool); keep[2, 5] = False
    for f in ("X", "U", "x_final"):
        assert np.array_equal(res[f][keep], clean[f][keep]), f
    assert res["rows"][keep].tobytes() == clean["rows"][keep].tobytes() and res["extra"][keep].tobytes() == clean["extra"][keep].tobytes()
    assert (clean["rows"]["first_bad"] == -1).all()
