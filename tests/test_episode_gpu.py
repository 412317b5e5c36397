"""MPC episodes (include/hsddp_episode.h; kernels k_episode_commit / k_episode_impact of cafe-mpc_amd/csrc/episode.hpp) on the device: bit for bit
against the same loop done by hand through the existing calls, parity with the oracle's loop (teacher-forced), a one-tick episode against
hsddp_mc_run, shards, no allocation when warm, and the refusals.  The fixture is the bound gait from window 11 (tests/episode_common.py): tick
index 1 ends exactly on the flight phase's touchdown."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import pkg
import sim_common as sc
import episode_common as ec

pytestmark = pytest.mark.gpu

EINVAL = -1
Dist = pkg.sim.Disturbance
ep = pkg.episode
MU, FZ_MIN = 0.6, 5.0
NOISE = dict(seed=20241222, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1)


def first_solve_setting(opt0):
    """The fixture's first solve: the shipped setting with three AL x four DDP iterations (the ticks use the runtime limits as shipped)."""
    opt0.max_AL_iter, opt0.max_DDP_iter = 3, 4
    return opt0


def same_handles(tag, a, b):
    ia, ib = a.info_arrays(), b.info_arrays()
    for k in ia:
        assert ia[k].tobytes() == ib[k].tobytes(), (tag, k, ia[k], ib[k])
    assert a.horizons == b.horizons
    for i in range(len(a.phases)):
        for f in ("K", "XBAR", "UBAR"):
            assert a.field(i, f).tobytes() == b.field(i, f).tobytes(), (tag, i, f)


def test_episode_is_the_manual_loop_bit_for_bit(hip_lib):
    """B = 5 (a partly filled wave), 4 ticks, noise + torque limit + fall height, force records on, a push at tick 1 step 0 that drops problem 1
    below the fall height and makes problem 3 diverge, the pending reset map at the end of tick 1.  The manual path: per tick a fresh Simulation
    with one sample, run with tick_seed, everything read to the host, fold_rows in numpy, set_initial_condition from the host for the problems
    still alive; at the touchdown tick the state behind the reset map comes from a second run over n_exec + 1 steps on the not-yet-moved window.
    That state is compared within sim_common.RTOL (another kernel applies the map in the episode) and the manual path then goes on from the
    episode's bits, so that everything after it can be held to equal bits as well."""
    B, T = 5, 4
    pdA, phA, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    pdM, phM = ec.bound_problem(pkg)[:2]
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, phA, B)
    A = pkg.MultiPhaseDDP(phA, batch=B); M = pkg.MultiPhaseDDP(phM, batch=B)
    epi = A.episode(n, T, keep_log=True); epi.set_grf(MU, FZ_MIN)
    epi.reset(x0); M.set_initial_condition(x0)
    A.solve(opt0); M.solve(opt0)
    same_handles("first solve", A, M)
    dist = Dist(**NOISE)
    state, ic, rows = x0.copy(), x0.copy(), ep.empty_rows(B)
    logX, logU, logY = np.zeros((B, T * n + 1, 36)), np.zeros((B, T * n, 12)), np.zeros((B, T * n, 12))
    n_imp, frozen_state = 0, None
    for t in range(T):
        kick, d_t = None, dist
        if t == 1:
            kick = np.zeros((B, 36)); kick[1, 2] = 0.07 - state[1, 2]; kick[3, 18] = 1e7
            d_t = dataclasses.replace(dist, kick_step=0)
        epi.advance(d_t, kick)
        # ---- the same tick by hand
        smap, pend = sc.step_map(phM, n), ec.pending_phase(phM, n)
        assert (pend >= 0) == (t == 1)
        dm = dataclasses.replace(d_t, seed=ep.tick_seed(dist.seed, t))
        k3 = None if kick is None else np.ascontiguousarray(kick[:, None])
        before = state.copy()
        sim = pkg.Simulation(M, 1, n, keep_traj=True); sim.set_grf(MU, FZ_MIN); sim.run(np.ascontiguousarray(before[:, None]), dist=dm, kick=k3)
        srows, xf = sim.rows(); extra = sim.extra(); grf, Y = sim.grf(); X, U = sim.traj(); sim.close()
        q, r = ep.step_weights(phM, smap); xr, ur = ep.step_refs(M, smap)
        live0 = rows["end_reason"] == 0
        rows = ep.fold_rows(rows, t, srows[:, 0], X[:, 0], U[:, 0], q, r, xr, ur, extra=extra[:, 0], grf=grf[:, 0], status=M.info_arrays()["status"])
        logX[live0, t * n:(t + 1) * n + 1] = X[live0, 0]; logU[live0, t * n:(t + 1) * n] = U[live0, 0]; logY[live0, t * n:(t + 1) * n] = Y[live0, 0]
        state[live0] = xf[live0, 0]
        live1 = rows["end_reason"] == 0
        erows, ex = epi.rows()
        if pend >= 0:
            sim2 = pkg.Simulation(M, 1, n + 1, keep_traj=True); sim2.run(np.ascontiguousarray(before[:, None]), dist=dm, kick=k3)
            post = sim2.traj()[0][:, 0, n]; sim2.close()
            assert np.array_equal(post[live1, :18], state[live1, :18]) and np.abs(post[live1, 18:] - state[live1, 18:]).max() > 1e-3      # a real impact
            sc.close("post-impact state", ex[live1], post[live1])
            assert np.array_equal(ex[live1, :18], post[live1, :18])
            state[live1] = ex[live1]; n_imp += 1
        ic[live1] = state[live1]
        M.set_initial_condition(ic)
        # ---- nothing is left out of the comparison
        for f in rows.dtype.names:
            if f != "track_cost":
                assert np.array_equal(erows[f], rows[f]), (t, f, erows[f], rows[f])
        rel = np.abs(erows["track_cost"] - rows["track_cost"]) / np.abs(rows["track_cost"])
        print(f"[episode] tick {t}: track_cost {erows['track_cost']}, rel diff to fold_rows {rel.max():.3e}, alive {live1.sum()}")
        assert rel.max() <= 1e-12
        assert np.array_equal(ex, state)
        eX, eU, eY = epi.log()
        assert np.array_equal(eX, logX) and np.array_equal(eU, logU) and np.array_equal(eY, logY)
        assert epi.status() == (t + 1, int(live1.sum()), n_imp)
        if t == 1:
            assert list(rows["end_reason"]) == [0, 2, 0, 1, 0] and rows["end_step"][1] == n and rows["end_step"][3] == n
            frozen_state = state[[1, 3]].copy()
        if t > 1:
            assert np.array_equal(ex[[1, 3]], frozen_state) and list(erows["steps"][[1, 3]]) == [2 * n, 2 * n]
        phA = ec.shift(pkg, A, phA, pdA); phM = ec.shift(pkg, M, phM, pdM)
        A.solve(opt_rt); M.solve(opt_rt)
        same_handles(f"tick {t}", A, M)      # also: the frozen problems' rows of the initial condition are what the manual path left them
    assert n_imp == 1 and list(rows["steps"]) == [T * n, 2 * n, T * n, 2 * n, T * n]
    # the rows of the handle's initial condition, read directly: a single-shooting rollout starts from them, so X[0] of phase 0 is the row itself.
    # Alive problems hold the last hand-off, the frozen ones still hold the state tick 1 began from (written behind tick 0, never since)
    ss = pkg.mhpc_ddp_setting(MS=0)
    A.hybrid_rollout(0.0, ss); M.hybrid_rollout(0.0, ss)
    icA, icM = A.field(0, "X")[:, 0], M.field(0, "X")[:, 0]
    assert np.array_equal(icM, ic) and np.array_equal(icA, ic)
    assert not np.array_equal(icA[1], frozen_state[0]) and not np.array_equal(icA[3], frozen_state[1]) and np.array_equal(icA[[0, 2, 4]], state[[0, 2, 4]])
    assert np.abs(logY).max() > 1.0 and (rows["n_sat"] >= 0).all() and np.isfinite(rows["track_cost"]).all()
    epi.close(); A.close(); M.close()


def test_episode_parity_with_the_oracle_loop_teacher_forced(hip_lib, oracle_lib):
    """Plain run, B = 4, 3 ticks.  At every tick the oracle handle starts from the GPU episode's state read back, so nothing compounds: the executed
    states and controls of tick 0 within sim_common.RTOL (the states start on the plan, so the policies' difference does not enter), those of the
    later ticks within the full-solve tolerance 1e-6 x scale, and the solver's counts identical at every tick.

    The oracle's reference rollout (sim_common.oracle_reference) overwrites X, U, XSIM and DEFECT of its handle, and a handle that goes on solving
    after it no longer follows the loop (its next policy moves by 1e-5 relative, measured).  So T + 1 oracle handles run the same loop in step;
    handle t gives the reference of tick t and is dropped, the last one is never rolled out by hand and gives the counts."""
    import importlib
    builder = importlib.import_module(pkg.__name__ + ".builder")
    B, T = 4, 3
    pdG, phG, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    pdO, phO = ec.bound_problem(pkg)[:2]
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, phG, B)
    G = pkg.MultiPhaseDDP(phG, batch=B)
    Os = []
    for _ in range(T + 1):
        O = pkg.Solver(oracle_lib, phO, batch=B)
        for i, p in enumerate(phO):
            O.set_nominal(i, p["Xbar"], p["Ubar"])
        O.set_initial_condition(x0); O.solve(opt0); Os.append(O)
    epi = G.episode(n, T, keep_log=True); epi.reset(x0)
    G.solve(opt0)
    ss = pkg.mhpc_ddp_setting(MS=0)
    n_imp = 0
    for t in range(T):
        x_now = np.ascontiguousarray(epi.rows()[1][:, None])
        pend = ec.pending_phase(phO, n)
        Xo, Uo, _ = sc.oracle_reference(Os[t], ss, x_now, sc.step_map(phO, n))
        if pend >= 0:      # entry n of the longer window is the state behind the reset map
            post = sc.oracle_reference(Os[t], ss, x_now, sc.step_map(phO, n + 1))[0][:, 0, n]
        epi.advance()
        eX, eU, _ = epi.log(); x_next = epi.rows()[1]
        gX, gU = eX[:, t * n:(t + 1) * n + 1], eU[:, t * n:(t + 1) * n]
        if t == 0:
            sc.close("tick 0 X", gX, Xo[:, 0]); sc.close("tick 0 U", gU, Uo[:, 0])
        else:
            for tag, a, ref in (("X", gX, Xo[:, 0]), ("U", gU, Uo[:, 0])):
                err, scale = np.abs(a - ref).max(), max(1.0, np.abs(ref).max())
                print(f"[episode] tick {t} {tag}: |diff| = {err:.3e}, scale {scale:.3e}, bound {1e-6 * scale:.3e}")
                assert err <= 1e-6 * scale
        if pend >= 0:
            n_imp += 1
            err, scale = np.abs(x_next - post).max(), max(1.0, np.abs(post).max())
            print(f"[episode] tick {t} post-impact state: |diff| = {err:.3e}, bound {1e-6 * scale:.3e}")
            assert err <= 1e-6 * scale and np.abs(x_next[:, 18:] - gX[:, n, 18:]).max() > 1e-3
        else:
            assert np.array_equal(x_next, gX[:, n])
        phG = ec.shift(pkg, G, phG, pdG); G.solve(opt_rt)
        m = pdO.update(); old = phO
        for O in Os[t + 1:]:
            O.set_initial_condition(x_next)
            phO, _ = builder.shift_solver_in_place(O, old, pdO, m, ubar_mode="zero")
            O.solve(opt_rt)
        ig, io = G.info_arrays(), Os[-1].info_arrays()
        for k in ("n_iters", "n_ls_iters", "n_reg_iters"):
            assert np.array_equal(ig[k], io[k]), (t, k, ig[k], io[k])
    assert n_imp == 1 and epi.status() == (T, B, 1)
    epi.close(); G.close()
    for O in Os:
        O.close()


@pytest.fixture(scope="module")
def trot6(hip_lib):
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    x0 = pkg.problems.wb_ensemble_x0(5, 9)
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(x0); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 2, 0.02, 0.2, seed=4)[:, 1]
    yield phases, s, np.ascontiguousarray(xs), x0
    s.close()


def test_one_tick_episode_is_hsddp_mc_run(trot6):
    """The same dist, one sample: rows, extras, final state and trajectory bit for bit (tick_seed(seed, 0) is the seed); also the plain run."""
    phases, s, xs, _ = trot6
    kick = np.zeros((5, 36)); kick[:, 19] = 0.2
    d = Dist(seed=77, sigma_u=0.2, sigma_q=1e-3, sigma_v=1e-2, u_max=8.0, fall_height=0.215, kick_step=3)
    for dist, k in ((d, kick), (None, None)):
        sim = pkg.Simulation(s, 1, 8, keep_traj=True)
        sim.run(np.ascontiguousarray(xs[:, None]), dist=dist, kick=None if k is None else np.ascontiguousarray(k[:, None]))
        srows, xf = sim.rows(); X, U = sim.traj(); extra = sim.extra() if dist is not None else None
        sim.close()
        e = s.episode(8, 1, keep_log=True); e.reset(xs); e.advance(dist, k)
        rows, x = e.rows(); eX, eU, eY = e.log()
        for f in ("dev_q", "dev_v", "min_height", "max_torque"):
            assert np.array_equal(rows[f], srows[f][:, 0]), f
        assert np.array_equal(x, xf[:, 0]) and np.array_equal(eX, X[:, 0]) and np.array_equal(eU, U[:, 0]) and not eY.any()
        assert (rows["steps"] == 8).all() and e.status()[0] == 1 and e.status()[2] == 0
        if dist is not None:
            assert np.array_equal(rows["n_sat"], extra["n_sat"][:, 0]) and (rows["n_sat"] > 0).any()
            fell = extra["first_fall"][:, 0] >= 0
            assert fell.any() and np.array_equal(rows["end_reason"], np.where(fell, 2, 0)) and np.array_equal(rows["end_step"][fell], extra["first_fall"][fell, 0])
        else:
            assert (rows["n_sat"] == 0).all() and (rows["end_reason"] == 0).all() and (srows["first_bad"] == -1).all()
        with pytest.raises(RuntimeError):
            e.advance(dist, k)      # max_ticks = 1
        e.close()
    s.set_initial_condition(trot6[3])


def test_episode_shard_reproduces_its_slice(hip_lib, trot6):
    """Problems [2, 5) in a handle of their own with first_problem = 2: rows and logs of the slice bit for bit, with the noise on, over two ticks of
    the same window (the second tick draws with tick_seed(seed, 1))."""
    phases, s, xs, x0 = trot6
    sh = pkg.MultiPhaseDDP(phases, batch=3); sh.set_initial_condition(np.ascontiguousarray(x0[2:])); sh.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    for i in range(len(phases)):
        assert sh.field(i, "K").tobytes() == s.field(i, "K", 2, 3).tobytes()      # the premise: a problem's solve does not depend on its batch
    d = Dist(seed=5, sigma_u=0.2, sigma_q=1e-3, sigma_v=1e-2, u_max=12.0)
    out = []
    for solver, x, first in ((s, xs, 0), (sh, xs[2:], 2)):
        e = solver.episode(5, 2, keep_log=True); e.set_grf(MU, FZ_MIN); e.reset(np.ascontiguousarray(x))
        dd = dataclasses.replace(d, first_problem=first)
        e.advance(dd); e.advance(dd)
        out.append((e.rows(), e.log())); e.close()
    (ra, xa), la = out[0]; (rb, xb), lb = out[1]
    assert ra[2:].tobytes() == rb.tobytes() and np.array_equal(xa[2:], xb)
    for a, b in zip(la, lb):
        assert np.array_equal(a[2:], b)
    assert not np.array_equal(la[1][2:, :5], la[1][2:, 5:]) and np.abs(la[2]).max() > 1.0
    # the second tick's noise is not the first's: the same tick run again with the plain seed differs
    e = s.episode(5, 2, keep_log=True); e.reset(xs); e.advance(d); x1 = e.rows()[1]; e.close()
    sim = pkg.Simulation(s, 1, 5, keep_traj=True); sim.run(np.ascontiguousarray(x1[:, None]), dist=d); U_same_seed = sim.traj()[1][:, 0]
    sim.run(np.ascontiguousarray(x1[:, None]), dist=dataclasses.replace(d, seed=ep.tick_seed(5, 1))); U_tick_seed = sim.traj()[1][:, 0]; sim.close()
    assert np.array_equal(la[1][:, 5:], U_tick_seed) and not np.array_equal(la[1][:, 5:], U_same_seed)
    sh.close(); s.set_initial_condition(x0)


def test_episode_allocates_nothing_when_warm(hip_lib):
    """hsddp_debug_malloc_count is flat from tick 4 on over 8 ticks with reconfigures and solves, and over a reset and a second episode."""
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    s = pkg.MultiPhaseDDP(ph, batch=2)
    x0 = ec.start_states(pkg, ph, 2)
    e = s.episode(n, 8); e.set_grf(MU, FZ_MIN); e.reset(x0); s.solve(first_solve_setting(opt0))
    d = Dist(seed=3, sigma_u=0.05, fall_height=0.05)
    counts = []
    for t in range(8):
        e.advance(d); ph = ec.shift(pkg, s, ph, pd); s.solve(opt_rt)
        counts.append(hip_lib.hsddp_debug_malloc_count())
    print(f"[episode] device allocations after each tick: {counts}")
    assert len(set(counts[3:])) == 1
    assert e.status()[0] == 8 and e.status()[2] >= 1
    e.reset(e.rows()[1])
    for t in range(3):
        e.advance(d); ph = ec.shift(pkg, s, ph, pd); s.solve(opt_rt)
    assert hip_lib.hsddp_debug_malloc_count() == counts[-1] and e.status()[0] == 3
    e.close(); s.close()


def test_episode_refusals_leave_everything_as_it_was(hip_lib):
    lib = pkg._abi.bind_episode(hip_lib)
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    x0 = pkg.problems.wb_ensemble_x0(5, 9)
    s = pkg.MultiPhaseDDP(phases, batch=5); s.set_initial_condition(x0); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=1))
    xs = np.ascontiguousarray(pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 2, 0.02, 0.2, seed=4)[:, 1])
    out = ctypes.c_void_p()
    assert lib.hsddp_episode_create(s.h, 0, 2, 0, ctypes.byref(out)) == EINVAL and lib.hsddp_episode_create(s.h, 2, 0, 0, ctypes.byref(out)) == EINVAL
    assert lib.hsddp_episode_create(None, 2, 2, 0, ctypes.byref(out)) == EINVAL and lib.hsddp_episode_create(s.h, 2, 2, 0, None) == EINVAL
    assert lib.hsddp_episode_create(s.h, 25, 2, 0, ctypes.byref(out)) == EINVAL      # more steps than the window has whole-body knots
    # a window whose first n_exec knots reach the single-rigid-body tail; an fp32 handle
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    wb = sum(p["desc"].horizon for p in ph if p["desc"].model == pkg.MODEL_WB)
    sb = pkg.MultiPhaseDDP(ph, batch=1)
    assert ph[-1]["desc"].model == pkg.MODEL_SRB and lib.hsddp_episode_create(sb.h, wb + 1, 2, 0, ctypes.byref(out)) == EINVAL
    assert lib.hsddp_episode_create(sb.h, wb, 2, 0, ctypes.byref(out)) == 0
    lib.hsddp_episode_destroy(out); sb.close()
    s32 = pkg.Solver(hip_lib, pkg.problems.hkd_trot_problem(horizons=(4, 4, 4, 4)), batch=1, precision=pkg.PREC_F32)
    assert lib.hsddp_episode_create(s32.h, 2, 2, 0, ctypes.byref(out)) == EINVAL
    s32.close()

    e = s.episode(4, 2, keep_log=False)
    good = Dist(seed=1, sigma_u=0.1, fall_height=0.1, kick_step=1)
    kick = np.zeros((5, 36)); kick[:, 19] = 0.1
    adv = lambda d, k=None: lib.hsddp_episode_advance(e.e, None if d is None else ctypes.byref(d.to_c()), None if k is None else k.ctypes.data, 0)
    snap = lambda: (e.rows()[0].tobytes(), e.rows()[1].tobytes(), e.status())
    assert adv(good) == EINVAL      # no reset yet
    e.reset(xs); e.advance(good, kick)
    before = snap()
    assert before[2][0] == 1
    mallocs = hip_lib.hsddp_debug_malloc_count()
    for ch in (dict(sigma_u=-0.1), dict(sigma_q=np.nan), dict(sigma_v=np.inf), dict(u_max=np.nan), dict(fall_height=-np.inf), dict(first_problem=-1)):
        assert adv(Dist(**{**good.__dict__, **ch})) == EINVAL, ch
    for ks in (-1, 4, 5):      # kick_step outside the tick
        assert adv(Dist(**{**good.__dict__, "kick_step": ks}), kick) == EINVAL, ks
    assert adv(None, kick) == EINVAL and lib.hsddp_episode_advance(None, None, None, 0) == EINVAL      # a kick without its step; a NULL object
    assert lib.hsddp_episode_reset(e.e, None, 0) == EINVAL and lib.hsddp_episode_reset(None, xs.ctypes.data, 0) == EINVAL
    rows = np.zeros(5, dtype=pkg._abi.EPISODE_ROW_DTYPE); buf = np.zeros((5, 9, 36))
    for b0, nb in ((-1, 1), (0, 0), (0, 6), (5, 1), (4, 2)):
        assert lib.hsddp_episode_get_rows(e.e, b0, nb, rows.ctypes.data, None) == EINVAL, (b0, nb)
    assert lib.hsddp_episode_get_rows(e.e, 0, 5, None, None) == EINVAL and lib.hsddp_episode_get_rows(None, 0, 5, rows.ctypes.data, None) == EINVAL
    assert lib.hsddp_episode_get_log(e.e, 0, 5, buf.ctypes.data, None, None) == EINVAL      # created without keep_log
    assert lib.hsddp_episode_status(None, None, None, None) == EINVAL
    assert lib.hsddp_episode_device_state(None) is None and lib.hsddp_episode_sim(None) is None and e.state() != 0
    # the window moved to one with fewer leading whole-body knots than n_exec: refused, and accepted again once it is long enough
    assert snap() == before and hip_lib.hsddp_debug_malloc_count() == mallocs      # nothing changed, nothing allocated
    s.reconfigure(pkg.problems.wb_trot_problem(schedule=((1, 1, 1, 1),), horizons=(3,)), [0], [0])
    mallocs = hip_lib.hsddp_debug_malloc_count()      # (a first hsddp_reconfigure lays out its arena)
    assert adv(good) == EINVAL and adv(None) == EINVAL
    assert snap() == before and hip_lib.hsddp_debug_malloc_count() == mallocs
    s.reconfigure(phases[:2], [0, -1], [0, 0])
    assert adv(good) == 0 and e.status()[0] == 2
    after = snap()
    assert adv(good) == EINVAL and adv(None) == EINVAL and snap() == after      # tick == max_ticks
    e.close(); s.close()


def test_cpp_episode_loop_matches_the_python_path(hip_lib, tmp_path):
    """tests/cpp/episode_loop.cpp built against libhsddp_hip.so and run for 4 ticks (B = 3, actuator noise and a fall height): per-tick iterations,
    alive counts and the rows equal the Python path's (episode.run_mhpc)."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    B, T = 3, 4
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, ph, B)
    d = Dist(seed=11, sigma_u=0.1, fall_height=0.1)
    exe = tmp_path / "episode_loop"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "episode_loop.cpp"), "-L", os.path.join(ROOT, "cafe-mpc_amd"), "-lhsddp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cafe-mpc_amd"), "-o", str(exe)])
    (tmp_path / "opt.bin").write_bytes(bytes(opt0)); (tmp_path / "x0.bin").write_bytes(x0.tobytes())
    out = json.loads(subprocess.check_output([str(exe), ec.TREE, "bound", str(tmp_path / "opt.bin"), str(tmp_path / "x0.bin"), str(B), str(ec.START_WINDOW), str(T),
                                              repr(d.sigma_u), repr(d.fall_height), str(d.seed)], timeout=120))
    s = pkg.MultiPhaseDDP(ph, batch=B)
    e = s.episode(n, T); e.reset(x0); s.solve(opt0)
    res = ep.run_mhpc(s, pd, ph, opt_rt, T, dist=d, episode=e)
    rows, x = e.rows()
    assert out["n_exec"] == n and [t["iters"] for t in out["per_tick"]] == res["n_iters"].tolist() and [t["alive"] for t in out["per_tick"]] == res["alive"].tolist()
    assert np.allclose([t["cost"] for t in out["per_tick"]], res["cost"], rtol=1e-9)
    assert out["per_tick"][-1]["impacts"] == e.status()[2] == 1
    for b in range(B):
        for f, v in out["rows"][b].items():
            assert v == rows[f][b], (b, f, v, rows[f][b])
    assert np.array_equal(np.array(out["x_now"]).reshape(B, 36), x) and (rows["steps"] == T * n).all()
    e.close(); s.close()
