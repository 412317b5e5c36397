"""Unilateral ground contact (include/hsddp_contact.h; kernels k_sim_quad_uni, k_sim_quad_mc_uni, k_sim_quad_mc0_uni of cafe-mpc_amd/csrc/hsddp_uni.hip)
on the device: the cases of tests/uni_common.py against the reference walk with the device's own policy, the invariants of the outputs, a partial
wave, contained divergence, toggling and the prefix property, refusals and allocation, and episodes with F carried from tick to tick."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import sim_common as sc
import mc_common as mc
import grf_common as gc
import sub_common as sub
import uni_common as un

pytestmark = pytest.mark.gpu

EINVAL = -1
MU = 0.6
FIELDS = ("X", "U", "XSIM", "DEFECT", "K", "XBAR", "UBAR")
Dist = pkg.sim.Disturbance
ep = pkg.episode
INTS = ("first_release", "n_release", "n_land", "n_free", "free_final")


@pytest.fixture(scope="module")
def trot12(oracle_lib, hip_lib):
    """trot12 of tests/test_substep_gpu.py: trot 4 x 12, B = 4, 3 AL x 4 DDP, R = 8 samples around Xbar[0]; the policy rows of the DEVICE handle."""
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


def test_no_event_is_the_bilateral_run(trot12, oracle_lib):
    """Case 1: fz_rel = -1e9, S = 3, records on (k_sim_quad_uni) against the bilateral records run at S = 3 (k_sim_quad_grf_sub) and against the
    bilateral reference, at the rollout tolerance; whether the two runs are bit-identical is printed.  All new counters are 0."""
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    res = un.library_run(pkg, sg, xs, 48, 3, -1e9, 0.0, mu=MU)
    base = sg.simulate(xs, 48, keep_traj=True, grf=(MU, 0.0), substeps=3)
    same = all(res[f].tobytes() == base[f].tobytes() for f in base)
    print(f"[uni] gpu no event: bit-identical to the bilateral run: {same}")
    c = res.pop("contact")
    ref = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs, 3)
    sub.compare_case("gpu uni no event S=3", pkg, res, ref, mc.xbar_window(pol, smap), gc.contact_of(phases, smap), MU, 0.0)
    for f in ("X", "U", "x_final", "Y"):
        sc.close(f"gpu uni against bilateral {f}", res[f], base[f])
    assert np.array_equal(res["grf"]["n_slip"], base["grf"]["n_slip"]) and np.array_equal(res["grf"]["first_slip"], base["grf"]["first_slip"])
    assert (c["first_release"] == -1).all() and not c["n_release"].any() and not c["n_land"].any() and not c["n_free"].any() and not c["free_final"].any() and not c["max_lift"].any()


@pytest.mark.parametrize("case,S", un.CASES)
def test_contact_cases_match_the_reference(trot12, oracle_lib, case, S):
    """Cases 2 - 6 of uni_common.case_setup: flight at S = 1 and 4 (k_sim_quad_mc0_uni), roll under noise (k_sim_quad_mc_uni), the partial wave at
    S = 5 and the contained divergence, against the reference walk; non-vacuity and the cap of one left-out sample asserted on the reference first;
    then the invariants of the device outputs."""
    phases, sg, xs, pol = trot12
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs)
    B = x0.shape[0]
    if B == 4:
        s, polB = sg, pol
    else:      # fewer problems: a handle of that batch with the same problems, its own policy rows
        s = pkg.MultiPhaseDDP(phases, batch=B)
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)[:B]); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
        polB = mc.policy_of(s)
    ref = un.oracle_walk_uni(pkg, oracle_lib, phases, polB, smap, x0, S, fz_rel, zg, d, k)
    un.assert_case_is_not_vacuous(case, ref, gc.contact_of(phases, smap))
    res = un.library_run(pkg, s, x0, 48, S, fz_rel, zg, d, k, MU)
    assert res["contact"].shape == x0.shape[:2] and res["Y"].shape == x0.shape[:2] + (48, 12)
    un.compare_case(f"gpu {case} S={S}", pkg, res, ref, mc.xbar_window(polB, smap), MU, 0.0, fz_rel)
    un.invariants(f"gpu {case} S={S}", res, fz_rel, gc.force_bound(ref["Y"]))
    if case == "divergence":      # the failing sample keeps the state behind substep 0 of step 5: not the state the step began with
        assert res["rows"]["first_bad"][1, 1] == 5 and not np.array_equal(res["x_final"][1, 1], res["X"][1, 1, 5])
        assert np.array_equal(res["X"][1, 1, 6:], np.broadcast_to(res["x_final"][1, 1], (43, 36)))
        sc.close("kept state", res["x_final"][1, 1], ref["X"][1, 1, -1], scale=float(np.abs(ref["X"][1, 1, -1]).max()))
        assert np.array_equal(res["contact"][INTS[1]][1, 1], ref["rows"][INTS[1]][1, 1])
    if s is not sg:
        s.close()


def collect(sim, disturbed, contact):
    rows, xf = sim.rows(); X, U = sim.traj()
    out = dict(rows=rows, x_final=xf, X=X, U=U)
    if disturbed:
        out["extra"] = sim.extra()
    if contact:
        out["contact"] = sim.contact_rows()
    return out


def test_toggling_and_prefix(trot12):
    """Case 7 on one object, for the flight case (no noise) and the roll case (noise), S = 4: on, off, on.  The off run is bit-identical to a fresh
    object's; the two on runs are bit-identical; and the 24-step run with the rule on is the first 24 steps of the 48-step one."""
    phases, sg, xs, pol = trot12
    for case in ("flight", "roll"):
        x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs)
        fresh = pkg.Simulation(sg, 8, 48, keep_traj=True); fresh.set_substeps(4)
        fresh.run(x0, dist=d, kick=k); want_off = collect(fresh, True, False); fresh.close()
        sim = pkg.Simulation(sg, 8, 48, keep_traj=True); sim.set_substeps(4)
        assert sim.contact == (False, 0.0, 0.0)
        sim.set_contact(fz_rel, zg); assert sim.contact == (True, fz_rel, zg)
        sim.run(x0, dist=d, kick=k); on1 = collect(sim, True, True)
        sim.clear_contact(); assert sim.contact[0] is False
        sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, False), want_off)
        with pytest.raises(RuntimeError):
            sim.contact_rows()                      # the last run had the rule off
        sim.set_contact(fz_rel, zg)
        sim.run(x0, dist=d, kick=k); same_bits(collect(sim, True, True), on1)
        assert on1["contact"]["n_release"].sum() > 0 and not np.array_equal(on1["X"], want_off["X"])
        sim.close()
    x0, d, k, fz_rel, zg = un.case_setup(pkg, "roll", xs)
    d = dataclasses.replace(d, kick_step=16)      # inside both windows
    long = un.library_run(pkg, sg, x0, 48, 4, 0.0, zg, d, k, MU)
    short = un.library_run(pkg, sg, x0, 24, 4, 0.0, zg, d, k, MU)
    assert short["contact"]["n_release"].sum() > 0
    assert np.array_equal(long["X"][:, :, :24], short["X"][:, :, :24]) and np.array_equal(long["U"][:, :, :24], short["U"]) and np.array_equal(long["Y"][:, :, :24], short["Y"])
    assert np.array_equal(long["X"][:, :, 24, :18], short["X"][:, :, 24, :18])      # (entry 24 of the long run lies behind a reset map: positions stay)


def snapshot(s):
    return {(i, f): s.field(i, f) for i in range(len(s.phases)) for f in FIELDS}


def test_contact_refusals_allocation_and_handle(hip_lib):
    """Case 8: HSDDP_EINVAL with nothing changed, hsddp_contact_get_params, the allocation count and the handle left as it was."""
    lib = pkg._abi.bind_contact(hip_lib)
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(pkg.problems.wb_ensemble_x0(5, 9)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=4)
    before = snapshot(s)
    sim = pkg.Simulation(s, 3, 20, keep_traj=True)
    sim.run(xs); first = collect(sim, False, False)
    on, f, z = ctypes.c_int(-7), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_contact_get_params(sim.s, ctypes.byref(on), ctypes.byref(f), ctypes.byref(z)) == 0 and (on.value, f.value, z.value) == (0, 0.0, 0.0)
    for bad in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0), (0.0, np.nan)):
        assert lib.hsddp_contact_set(sim.s, 1, *bad) == EINVAL and lib.hsddp_contact_set(sim.s, 0, *bad) == EINVAL
    assert lib.hsddp_contact_set(None, 1, 0.0, 0.0) == EINVAL and lib.hsddp_contact_get_params(None, ctypes.byref(on), ctypes.byref(f), ctypes.byref(z)) == EINVAL
    assert lib.hsddp_contact_get_params(sim.s, None, ctypes.byref(f), ctypes.byref(z)) == EINVAL and lib.hsddp_contact_get_params(sim.s, ctypes.byref(on), None, ctypes.byref(z)) == EINVAL
    rows = np.zeros((5, 3), dtype=pkg._abi.CONTACT_ROW_DTYPE)
    assert lib.hsddp_contact_get(sim.s, 0, 5, rows.ctypes.data) == EINVAL      # no run with the rule yet
    assert lib.hsddp_contact_set(sim.s, 0, 0.0, 0.0) == 0                      # off on an object that never had it on: nothing to do
    assert hip_lib.hsddp_debug_malloc_count() == mallocs and sim.contact == (False, 0.0, 0.0)
    sim.run(xs); same_bits(collect(sim, False, False), first)                  # the refused calls changed nothing
    sim.set_contact(-3.0, 0.01); assert sim.contact == (True, -3.0, 0.01)
    m1 = hip_lib.hsddp_debug_malloc_count(); assert m1 > mallocs               # the first on allocates
    assert lib.hsddp_contact_set(sim.s, 1, np.nan, 0.0) == EINVAL and sim.contact == (True, -3.0, 0.01)
    sim.run(xs); one = collect(sim, False, True)
    assert lib.hsddp_contact_get(sim.s, 0, 5, None) == EINVAL and lib.hsddp_contact_get(sim.s, 3, 3, rows.ctypes.data) == EINVAL and lib.hsddp_contact_get(sim.s, -1, 2, rows.ctypes.data) == EINVAL
    assert lib.hsddp_contact_get(None, 0, 5, rows.ctypes.data) == EINVAL
    assert np.array_equal(sim.contact_rows(1, 2), one["contact"][1:3])
    with pytest.raises(RuntimeError):
        sim.grf()                                                              # hsddp_grf_get keeps answering as without the rule: the records are off
    sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.set_grf(MU); sim.run(xs); sim.grf(); sim.set_substeps(3); sim.run(xs)      # first uses of the others
    m2 = hip_lib.hsddp_debug_malloc_count()
    sim.set_contact(0.0, 0.0); sim.run(xs); sim.clear_contact(); sim.run(xs); sim.set_contact(-3.0, 0.01); sim.set_substeps(1); sim.set_grf(0.0); sim.run(xs)
    again = collect(sim, False, True)
    sim.run(xs, dist=Dist(seed=3, u_max=17.0)); sim.run(xs, dist=Dist(seed=3, sigma_u=0.1)); sim.contact_rows()
    assert hip_lib.hsddp_debug_malloc_count() == m2                            # later calls and all runs allocate nothing
    same_bits(again, one)
    after = snapshot(s)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k                    # the handle is bit for bit what it was
    res = s.simulate(xs, 20, keep_traj=True, contact=(-3.0, 0.01))             # the one-off path
    same_bits(res, one)
    sim.close(); s.close()


def test_one_tick_episode_is_the_run(trot12):
    """Case 9a: one sample per problem, 12 steps, S = 4, the rule on through hsddp_episode_sim: rows, state, log and contact rows bit for bit those
    of hsddp_mc_run on a simulation object (an upward kick at step 4 under the torque limit: releases inside the tick, asserted)."""
    phases, sg, xs, pol = trot12
    x1 = np.ascontiguousarray(xs[:, 7])
    d = Dist(seed=mc.SEED, u_max=8.0, kick_step=4)
    k = np.zeros((4, 36)); k[:, 20] = 1.6
    sim = pkg.Simulation(sg, 1, 12, keep_traj=True); sim.set_substeps(4); sim.set_grf(MU); sim.set_contact(un.FZ_REL, 0.0)
    sim.run(np.ascontiguousarray(x1[:, None]), dist=d, kick=np.ascontiguousarray(k[:, None]))
    srows, xf = sim.rows(); X, U = sim.traj(); g, Y = sim.grf(); c = sim.contact_rows(); sim.close()
    assert (c["n_release"] > 0).any()
    e = sg.episode(12, 1, keep_log=True); e.set_substeps(4); e.set_grf(MU); e.set_contact(un.FZ_REL, 0.0)
    e.reset(x1); e.advance(d, k)
    rows, x_now = e.rows(); eX, eU, eY = e.log()
    for f in ("dev_q", "dev_v", "min_height", "max_torque"):
        assert np.array_equal(rows[f], srows[f][:, 0]), f
    for f in ("min_fz", "min_cone", "max_fz", "n_slip", "first_slip"):
        assert np.array_equal(rows[f], g[f][:, 0]), f
    assert np.array_equal(x_now, xf[:, 0]) and np.array_equal(eX, X[:, 0]) and np.array_equal(eU, U[:, 0]) and np.array_equal(eY, Y[:, 0])
    assert e.contact_rows().tobytes() == c[:, 0].tobytes()
    e.close()
    sg.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222))


def test_three_tick_episode_carries_f(hip_lib, oracle_lib):
    """Case 9b: trot 4 x 12, B = 4, n_exec = 12, three ticks with hsddp_reconfigure and a solve between them, S = 4, torque limit, an upward kick
    at step 9 of tick 0 only (later ticks: a zero kick), sized so that a robot ends tick 0 with a free foot (asserted).  Every tick is compared with
    the reference walked from the episode's state before the tick, with the policy read from the handle and the REFERENCE's F handed from tick to
    tick.  hsddp_episode_reset clears F."""
    B, T, n = 4, 3, 12
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    x0 = pkg.problems.wb_ensemble_x0(B, 20241222)
    opt0, opt_rt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4), pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    A = pkg.MultiPhaseDDP(phases, batch=B)
    epi = A.episode(n, T, keep_log=True); epi.set_grf(MU); epi.set_substeps(4); epi.set_contact(un.FZ_REL, 0.0)
    epi.reset(x0); A.solve(opt0)
    dist = Dist(seed=mc.SEED, u_max=8.0, kick_step=9)
    kick = np.zeros((B, 36)); kick[:, 20] = np.linspace(0.8, 1.6, B)
    ident = (list(range(len(phases))), [0] * len(phases))
    smap = sc.step_map(phases, n)
    state, F = x0.copy(), np.zeros((B, 1, 4), dtype=bool)
    for t in range(T):
        pol = mc.policy_of(A)
        kt = kick if t == 0 else np.zeros_like(kick)
        ref = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap, np.ascontiguousarray(state[:, None]), 4, un.FZ_REL, 0.0,
                                 dataclasses.replace(dist, seed=ep.tick_seed(dist.seed, t)), np.ascontiguousarray(kt[:, None]), F0=F)
        live0 = epi.rows()[0]["end_reason"] == 0
        epi.advance(dist, kt)
        erows, x_now = epi.rows(); c = epi.contact_rows()
        near = un.near_samples(f"episode tick {t}", ref)[:, 0]
        ok = live0 & ~near & (ref["first_bad"][:, 0] < 0)
        print(f"[uni] episode tick {t}: free_final {c['free_final']}, n_release {c['n_release']}, n_land {c['n_land']}, compared {int(ok.sum())} of {B}")
        assert ok.sum() >= B - 1
        for f in INTS:
            assert np.array_equal(c[f][ok], ref["rows"][f][ok, 0]), (t, f, c[f], ref["rows"][f][:, 0])
        sc.close(f"episode tick {t} state", x_now[ok], ref["X"][ok, 0, -1])
        if t == 0:
            assert (ref["F"][:, 0].any(axis=-1) & ok).any(), "no robot ends tick 0 with a free foot"
        if t == 1:
            assert (ref["rows"]["n_land"][:, 0] + ref["rows"]["n_free"][:, 0] > 0)[ok].any()      # the F of tick 0 did act in tick 1
        state, F = x_now, ref["F"]
        A.reconfigure(phases, *ident); A.solve(opt_rt)
    # hsddp_episode_reset clears F: a tick that leaves a foot free, reset, the same tick again under the same policy - the same bits, which a
    # carried F would change; and that tick is the reference's with F empty
    epi.reset(x0); epi.advance(dist, kick)
    x_a, c_a = epi.rows()[1].copy(), epi.contact_rows().copy()
    assert c_a["free_final"].any()
    epi.reset(x0); epi.advance(dist, kick)
    assert np.array_equal(epi.rows()[1], x_a) and epi.contact_rows().tobytes() == c_a.tobytes()
    ref = un.oracle_walk_uni(pkg, oracle_lib, phases, mc.policy_of(A), smap, np.ascontiguousarray(x0[:, None]), 4, un.FZ_REL, 0.0, dist, np.ascontiguousarray(kick[:, None]))
    ok = ~un.near_samples("episode after reset", ref)[:, 0]
    for f in INTS:
        assert np.array_equal(c_a[f][ok], ref["rows"][f][ok, 0]), f
    epi.close(); A.close()
