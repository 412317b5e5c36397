"""Policy latency of the MPC episodes (include/hsddp_latency.h; kernel k_episode_latency of cafe-mpc_amd/csrc/episode.hpp) on the device: the composed
rows and the stash bit for bit against episode.compose_policy, delay 0 against an episode that never heard of latency, mixed delays across the
touchdown of the bound gait against the host build of the walk on the composed rows (teacher-forced), the other walk families, the refusals, and
the C++ harness.  All compared runs use identical disturbances."""
import ctypes
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc
import episode_common as ec

pytestmark = pytest.mark.gpu

EINVAL = -1
Dist = pkg.sim.Disturbance
ep = pkg.episode
MU, FZ_MIN = 0.6, 5.0
NOISE = dict(seed=20241222, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1)      # those of tests/test_episode_gpu.py


def first_solve_setting(opt0):
    opt0.max_AL_iter, opt0.max_DDP_iter = 3, 4
    return opt0


def same_policy(tag, got, rows):
    """Episode.applied_policy() against rows [B, n, 516], bit for bit."""
    for name, a, b in zip(("Xe", "Ue", "Ke"), got, ep.split_policy(rows)):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes(), (tag, name)


def trot_handle(B, x0_seed=9):
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6))
    x0 = pkg.problems.wb_ensemble_x0(B, x0_seed)
    s = pkg.MultiPhaseDDP(phases, batch=B); s.set_initial_condition(x0); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    xs = np.ascontiguousarray(pkg.problems.perturbed_states(s.field(0, "XBAR")[:, 0], 2, 0.02, 0.2, seed=4)[:, 1])
    return phases, s, xs, x0


def two_ticks_on_one_window(s, e, phases, xs, x0, n, delay, dist=None):
    """Tick 0, then another policy on the SAME window (a solve from other initial states: an odd use that isolates the kernel), then tick 1.  Returns the
    rows the handle held at the two ticks over the long map, [B, n + D, 516] each."""
    D = int(np.max(delay))
    lmap = sc.step_map(phases, n + D)
    e.reset(xs)
    rows0 = ep.policy_rows(s, lmap)
    e.advance(dist)
    same_policy("tick 0", e.applied_policy(), rows0[:, :n])      # fresh: nothing was stashed yet
    s.set_initial_condition(np.ascontiguousarray(x0 + 0.01)); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=1))
    rows1 = ep.policy_rows(s, lmap)
    assert not np.array_equal(rows0, rows1)
    e.advance(dist)
    return rows0, rows1


def test_composition_and_stash_bit_for_bit(hip_lib):
    """B = 17 (two waves of the walk, the second partly filled), n_exec = 3, delays cycling 0 .. 3 (D = n_exec), two phases inside the long map."""
    B, n = 17, 3
    phases, s, xs, x0 = trot_handle(B)
    delay = np.arange(B, dtype=np.int32) % 4
    e = s.episode(n, 3, keep_log=True); e.set_latency(delay)
    lr = e.latency_rows()
    assert np.array_equal(lr["delay"], delay) and not lr["n_stale"].any()
    rows0, rows1 = two_ticks_on_one_window(s, e, phases, xs, x0, n, delay)
    alive0 = np.ones(B, dtype=bool)      # the plain walk of a solved policy: nobody diverges in tick 0 (asserted below through the rows)
    want = ep.compose_policy(rows0[:, n:], rows1[:, :n], delay, True)
    same_policy("tick 1", e.applied_policy(), want)
    assert not np.array_equal(want[3], rows1[3, :n]) and np.array_equal(want[4], rows1[4, :n])
    same_policy("tick 1 slice", e.applied_policy(5, 7), want[5:12])
    rows, _ = e.rows(); lr = e.latency_rows()
    assert (rows["end_reason"] == 0).all() and alive0.all()
    assert np.array_equal(lr["delay"], delay) and np.array_equal(lr["n_stale"], delay)
    assert np.array_equal(e.latency_rows(6, 3)["n_stale"], delay[6:9])
    # the stash the second tick wrote is what a third one applies: the same window and policy again
    e.advance()
    same_policy("tick 2", e.applied_policy(), ep.compose_policy(rows1[:, n:], rows1[:, :n], delay, True))
    assert np.array_equal(e.latency_rows()["n_stale"], 2 * delay)
    # a reset keeps the delays, zeroes the counters and forgets the stash
    e.reset(xs); lr = e.latency_rows()
    assert np.array_equal(lr["delay"], delay) and not lr["n_stale"].any()
    e.advance()
    same_policy("tick 0 again", e.applied_policy(), rows1[:, :n])
    assert not e.latency_rows()["n_stale"].any()
    e.close(); s.close()


def test_delay_zero_is_todays_episode(hip_lib):
    """The bound gait, B = 5, T = 4, noise + torque limit + fall height, force records, the push of the manual-loop test at tick 1 (robot 1 falls, robot 3
    diverges), the pending reset map at the end of tick 1: a handle whose episode has set_latency(0) and one that never set it, bit for bit."""
    B, T = 5, 4
    pdA, phA, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    pdL, phL = ec.bound_problem(pkg)[:2]
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, phA, B)
    A = pkg.MultiPhaseDDP(phA, batch=B); L = pkg.MultiPhaseDDP(phL, batch=B)
    eA = A.episode(n, T, keep_log=True); eA.set_grf(MU, FZ_MIN); eA.reset(x0)
    eL = L.episode(n, T, keep_log=True); eL.set_grf(MU, FZ_MIN); eL.set_latency(0); eL.reset(x0)
    A.solve(opt0); L.solve(opt0)
    dist = Dist(**NOISE)

    def same(tag):
        ia, ib = A.info_arrays(), L.info_arrays()
        for k in ia:
            assert ia[k].tobytes() == ib[k].tobytes(), (tag, k)
        for i in range(len(A.phases)):
            for f in ("K", "XBAR", "UBAR"):
                assert A.field(i, f).tobytes() == L.field(i, f).tobytes(), (tag, i, f)
        (ra, xa), (rb, xb) = eA.rows(), eL.rows()
        assert ra.tobytes() == rb.tobytes() and xa.tobytes() == xb.tobytes(), tag
        for a, b in zip(eA.log(), eL.log()):
            assert a.tobytes() == b.tobytes(), tag
        assert eA.status() == eL.status(), tag
        return ra

    same("first solve")
    for t in range(T):
        kick, d_t = None, dist
        if t == 1:
            state = eA.rows()[1]
            kick = np.zeros((B, 36)); kick[1, 2] = 0.07 - state[1, 2]; kick[3, 18] = 1e7
            d_t = dataclasses.replace(dist, kick_step=0)
        smap = sc.step_map(phL, n)
        fresh = ep.policy_rows(L, smap)
        eA.advance(d_t, kick); eL.advance(d_t, kick)
        rows = same(f"tick {t} advance")
        same_policy(f"tick {t}", eL.applied_policy(), fresh)
        if t == 1:
            assert list(rows["end_reason"]) == [0, 2, 0, 1, 0] and eA.status()[2] == 1
        phA = ec.shift(pkg, A, phA, pdA); phL = ec.shift(pkg, L, phL, pdL)
        A.solve(opt_rt); L.solve(opt_rt)
        same(f"tick {t} solve")
    assert not eL.latency_rows()["n_stale"].any()
    eA.close(); eL.close(); A.close(); L.close()


def shadow_walk(sim_lib, phases, smap, rows_b, x0):
    """The host build of the plain walk on ONE robot's composed rows [n, 516]: one phase of one knot per step with the step's own schedule, the map
    (s, 0, reset of step s) - what the walk kernel is launched on.  Returns (X [n + 1, 36], U [n, 12], row [5])."""
    n = smap.shape[1]
    D = [phases[int(p)]["desc"] for p in smap[0]]
    hor = np.ones(n, dtype=np.int32); dt = np.array([d.dt for d in D]); al = np.array([d.BG_alpha for d in D])
    ct = np.array([[d.contact[l] for l in range(4)] for d in D], dtype=np.int32)
    td = np.array([[1 if (d.contact[l] == 0 and d.next_contact[l] == 1) else 0 for l in range(4)] for d in D], dtype=np.int32)
    xb = [np.ascontiguousarray(rows_b[s, :72]) for s in range(n)]; ub = [np.ascontiguousarray(rows_b[s, 72:84]) for s in range(n)]; kk = [np.ascontiguousarray(rows_b[s, 84:]) for s in range(n)]
    ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    wmap = np.ascontiguousarray(np.array([np.arange(n), np.zeros(n), smap[2]], dtype=np.int32))
    x0 = np.ascontiguousarray(x0.reshape(1, 36))
    xf = np.zeros((1, 36)); row = np.zeros((1, 5)); X = np.zeros((1, n + 1, 36)); U = np.zeros((1, n, 12))
    rc = sim_lib.sim_emu_run(n, ec.vp(hor), ec.vp(dt), ec.vp(al), ec.vp(ct), ec.vp(td), ptrs(xb), ptrs(ub), ptrs(kk), ctypes.c_double(3.1415), ec.vp(wmap), n, 1,
                             ec.vp(x0), ec.vp(xf), ec.vp(row), ec.vp(X), ec.vp(U))
    assert rc == 0
    return X[0], U[0], row[0]


def test_mixed_delays_across_the_touchdown(hip_lib, tmp_path):
    """The bound gait, plain walk, delays [0, 2, 0, 1, 2] (D = n_exec = 2), T = 4.  Tick 1 ends on the flight phase's touchdown, so the stale steps of
    tick 2 come from behind a reset map of the previous window.  Robots with delay 0 are bit for bit those of a plain episode run beside them; the
    delayed ones are checked per tick, teacher-forced: from the episode's state before the tick, compose_policy of the two field snapshots feeds the
    host build of the walk, and the tick's slice of the log agrees within sim_common.RTOL (host walk against device walk).  On every stale step the
    applied control differs from what the fresh row gives by more than that tolerance: the assertion an episode without latency fails."""
    B, T = 5, 4
    delay = np.array([0, 2, 0, 1, 2], dtype=np.int32); D = 2
    sim_lib = ec.build_sim_emu(tmp_path)
    pdP, phP, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    pdL, phL = ec.bound_problem(pkg)[:2]
    assert n == 2
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, phP, B)
    P = pkg.MultiPhaseDDP(phP, batch=B); L = pkg.MultiPhaseDDP(phL, batch=B)
    eP = P.episode(n, T, keep_log=True); eP.reset(x0)
    eL = L.episode(n, T, keep_log=True); eL.set_latency(delay); eL.reset(x0)
    P.solve(opt0); L.solve(opt0)
    zero = delay == 0
    stash, n_stale, impacts = None, np.zeros(B, dtype=np.int32), 0
    for t in range(T):
        lmap = sc.step_map(phL, n + D); smap = sc.step_map(phL, n)
        pend = ec.pending_phase(phL, n)
        cur = ep.policy_rows(L, lmap)
        x_before = eL.rows()[1]
        eP.advance(); eL.advance()
        eff = ep.compose_policy(stash, cur[:, :n], delay, t >= 1)
        same_policy(f"tick {t}", eL.applied_policy(), eff)
        if t >= 1:
            n_stale += delay
        assert np.array_equal(eL.latency_rows()["n_stale"], n_stale)
        (rP, xP), (rL, xL) = eP.rows(), eL.rows()
        lP, lL = eP.log(), eL.log()
        assert rP[zero].tobytes() == rL[zero].tobytes() and np.array_equal(xP[zero], xL[zero]), t
        for a, b in zip(lP, lL):
            assert np.array_equal(a[zero], b[zero]), t
        assert (rL["end_reason"] == 0).all()
        gX, gU = lL[0][:, t * n:(t + 1) * n + 1], lL[1][:, t * n:(t + 1) * n]
        for b in np.flatnonzero(~zero):
            X, U, row = shadow_walk(sim_lib, phL, smap, eff[b], x_before[b])
            sc.close(f"tick {t} robot {b} X", gX[b], X); sc.close(f"tick {t} robot {b} U", gU[b], U)
            for s in range(delay[b] if t >= 1 else 0):      # a stale step: the fresh row would have asked for another torque
                fr = cur[b, s]
                u_fresh = fr[72:84] + fr[84:].reshape(36, 12).T @ (gX[b, s] - fr[:36])
                diff, scale = np.abs(gU[b, s] - u_fresh).max(), max(1.0, np.abs(u_fresh).max())
                print(f"[latency] tick {t} robot {b} step {s}: |u_applied - u_fresh| = {diff:.3e}, tolerance of the comparison {sc.RTOL * scale:.3e}")
                assert diff > sc.RTOL * scale
        if pend >= 0:
            impacts += 1
            assert t == 1
        if t == 2:      # the stale rows of this tick were stashed at knots behind the reset map of window 12
            assert sc.step_map(prev_ph, n + D)[2][n - 1] == 1
        stash, prev_ph = cur[:, n:], phL
        phP = ec.shift(pkg, P, phP, pdP); phL = ec.shift(pkg, L, phL, pdL)
        P.solve(opt_rt); L.solve(opt_rt)
    assert impacts == 1 and eL.status() == (T, B, 1) and list(n_stale) == [0, 6, 0, 3, 6]
    # the delayed robots did not walk the plain episode's path
    assert not np.array_equal(eP.log()[1][~zero], eL.log()[1][~zero])
    eP.close(); eL.close(); P.close(); L.close()


@pytest.mark.parametrize("family", ["sub_grf", "uni", "plant"])
def test_every_launcher_family_sees_the_shadow_table(hip_lib, family):
    """B = 4, two ticks, delay 1, with sub-steps 2 and force records / unilateral contact / a plant table: the composed rows as in the first test, and
    dev_q of the rows recomputed from the log against the EFFECTIVE Xbar - which only a walk sent to the per-step table reproduces."""
    B, n = 4, 3
    phases, s, xs, x0 = trot_handle(B)
    e = s.episode(n, 2, keep_log=True)
    if family == "sub_grf":
        e.set_substeps(2); e.set_grf(MU, FZ_MIN)
    elif family == "uni":
        e.set_contact(0.0, 0.0)
    else:
        rows = pkg.sim.Plant.nominal(2).table(); rows[1, 0] *= 1.1
        e.set_plant(pkg.sim.Plant(rows, plant_of=np.array([0, 1, 0, 1], dtype=np.int32)))
    delay = np.ones(B, dtype=np.int32)
    e.set_latency(1)
    rows0, rows1 = two_ticks_on_one_window(s, e, phases, xs, x0, n, delay)
    eff1 = ep.compose_policy(rows0[:, n:], rows1[:, :n], delay, True)
    same_policy("tick 1", e.applied_policy(), eff1)
    assert np.array_equal(e.latency_rows()["n_stale"], delay)
    rows, _ = e.rows(); X, U, Y = e.log()
    assert (rows["end_reason"] == 0).all()
    dq = np.zeros(B); dq_fresh = np.zeros(B)
    for t, (eff, fresh) in enumerate(((rows0[:, :n], rows0[:, :n]), (eff1, rows1[:, :n]))):
        for tag, r, acc in (("eff", eff, dq), ("fresh", fresh, dq_fresh)):
            xbar = np.concatenate([r[:, :, :36], r[:, -1:, 36:72]], axis=1)      # [B, n + 1, 36]: the knot behind the last step closes the tick
            np.maximum(acc, np.abs(X[:, t * n:(t + 1) * n + 1, :18] - xbar[:, :, :18]).max(axis=(1, 2)), out=acc)
    print(f"[latency] {family}: dev_q {rows['dev_q']}, against the effective plan {dq}, against the fresh plan {dq_fresh}")
    assert np.array_equal(rows["dev_q"], dq)      # (the maximum may sit on a fresh step, so dq and dq_fresh may agree: the composed rows above are what tells the tables apart)
    if family == "sub_grf":
        assert np.abs(Y).max() > 1.0
    e.close(); s.close()


def test_latency_refusals_leave_everything_as_it_was(hip_lib):
    lib = pkg._abi.bind_latency(hip_lib)
    B, n = 5, 4
    phases, s, xs, x0 = trot_handle(B)
    e = s.episode(n, 6, keep_log=True)
    lrow = np.zeros(B, dtype=pkg._abi.LATENCY_ROW_DTYPE); buf = np.zeros((B, n, 432))
    good = np.array([0, 1, 2, 4, 1], dtype=np.int32)
    assert lib.hsddp_latency_set(None, 1, None, 1) == EINVAL and lib.hsddp_latency_get(None, 0, B, lrow.ctypes.data) == EINVAL
    assert lib.hsddp_latency_get(e.e, 0, B, lrow.ctypes.data) == EINVAL      # nothing was ever set
    assert lib.hsddp_latency_set(e.e, 1, None, n + 1) == EINVAL and lib.hsddp_latency_set(e.e, 1, None, -1) == EINVAL
    e.set_latency(good)
    for bad in ([0, 1, 2, 5, 1], [0, -1, 2, 4, 1]):
        assert lib.hsddp_latency_set(e.e, 1, np.array(bad, dtype=np.int32).ctypes.data, 0) == EINVAL
    assert np.array_equal(e.latency_rows()["delay"], good)
    assert lib.hsddp_latency_get_policy(e.e, 0, B, None, None, buf.ctypes.data) == EINVAL      # no tick with latency yet
    assert lib.hsddp_latency_get_policy(None, 0, B, None, None, buf.ctypes.data) == EINVAL
    e.reset(xs)
    assert lib.hsddp_latency_get_policy(e.e, 0, B, None, None, buf.ctypes.data) == EINVAL
    e.advance(); e.advance()
    for b0, nb in ((-1, 1), (0, 0), (0, 6), (5, 1), (4, 2)):
        assert lib.hsddp_latency_get(e.e, b0, nb, lrow.ctypes.data) == EINVAL and lib.hsddp_latency_get_policy(e.e, b0, nb, None, None, buf.ctypes.data) == EINVAL, (b0, nb)
    assert lib.hsddp_latency_get(e.e, 0, B, None) == EINVAL
    snap = lambda: (e.rows()[0].tobytes(), e.rows()[1].tobytes(), e.status(), e.latency_rows().tobytes(), [a.tobytes() for a in e.applied_policy()], [a.tobytes() for a in e.log()],
                    [s.field(i, f).tobytes() for i in range(len(s.phases)) for f in ("K", "XBAR", "UBAR")])
    before = snap()
    assert before[2][0] == 2 and np.array_equal(e.latency_rows()["n_stale"], good)
    # a window that leads with n_exec whole-body knots but not with n_exec + D: refused with latency on, with nothing changed and nothing allocated
    s.reconfigure(pkg.problems.wb_trot_problem(schedule=((1, 1, 1, 1),), horizons=(6,)), [0], [0])
    before = snap()      # (the reconfigure moved the handle's fields)
    mallocs = hip_lib.hsddp_debug_malloc_count()
    assert lib.hsddp_episode_advance(e.e, None, None, 0) == EINVAL      # 6 < 4 + 4
    assert snap() == before and hip_lib.hsddp_debug_malloc_count() == mallocs
    e.set_latency(2)      # 6 = 4 + 2
    assert lib.hsddp_episode_advance(e.e, None, None, 0) == 0 and e.status()[0] == 3
    assert not e.latency_rows()["n_stale"][0] and np.array_equal(e.latency_rows()["n_stale"], good)      # set_latency forgot the stash: a fresh tick
    e.set_latency(good)
    assert lib.hsddp_episode_advance(e.e, None, None, 0) == EINVAL
    e.clear_latency()      # without latency the same window is long enough
    assert lib.hsddp_episode_advance(e.e, None, None, 0) == 0 and e.status()[0] == 4
    e.close(); s.close()


def test_latency_allocates_nothing_when_warm(hip_lib):
    """hsddp_debug_malloc_count is flat from tick 4 on over 8 ticks with latency, reconfigures and solves, and over a reset and three more ticks."""
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    s = pkg.MultiPhaseDDP(ph, batch=2)
    x0 = ec.start_states(pkg, ph, 2)
    e = s.episode(n, 8); e.set_latency([1, 2]); e.reset(x0); s.solve(first_solve_setting(opt0))
    d = Dist(seed=3, sigma_u=0.05, fall_height=0.05)
    counts = []
    for t in range(8):
        e.advance(d); ph = ec.shift(pkg, s, ph, pd); s.solve(opt_rt)
        counts.append(hip_lib.hsddp_debug_malloc_count())
    print(f"[latency] device allocations after each tick: {counts}")
    assert len(set(counts[3:])) == 1 and e.status()[0] == 8
    e.reset(e.rows()[1])
    for t in range(3):
        e.advance(d); ph = ec.shift(pkg, s, ph, pd); s.solve(opt_rt)
    assert hip_lib.hsddp_debug_malloc_count() == counts[-1] and e.status()[0] == 3
    kt = s.kernel_times(max_n=64)      # one launch a tick, timed into the handle's kernel table like the commit
    assert kt["k_episode_latency"][1] == kt["k_episode_commit"][1] == 11
    e.clear_latency(); e.advance(d)
    kt = s.kernel_times(max_n=64)
    assert kt["k_episode_latency"][1] == 11 and kt["k_episode_commit"][1] == 12      # off: no extra kernel
    e.close(); s.close()


def test_latency_shard_reproduces_its_slice(hip_lib):
    """Problems [2, 5) in a handle of their own with first_problem = 2 and their own delays: rows, latency rows, logs and composed rows of the slice bit for
    bit, with the noise on, over two ticks of the same window (the second applies stale rows)."""
    B, n = 5, 5
    phases, s, xs, x0 = trot_handle(B)
    sh = pkg.MultiPhaseDDP(phases, batch=3); sh.set_initial_condition(np.ascontiguousarray(x0[2:])); sh.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2))
    for i in range(len(phases)):
        assert sh.field(i, "K").tobytes() == s.field(i, "K", 2, 3).tobytes()      # the premise: a problem's solve does not depend on its batch
    delay = np.array([0, 1, 2, 3, 1], dtype=np.int32)
    d = Dist(seed=5, sigma_u=0.2, sigma_q=1e-3, sigma_v=1e-2, u_max=12.0)
    out = []
    for solver, x, dl, first in ((s, xs, delay, 0), (sh, xs[2:], delay[2:], 2)):
        e = solver.episode(n, 2, keep_log=True); e.set_grf(MU, FZ_MIN); e.set_latency(dl); e.reset(np.ascontiguousarray(x))
        dd = dataclasses.replace(d, first_problem=first)
        e.advance(dd); e.advance(dd)
        out.append((e.rows(), e.log(), e.latency_rows(), e.applied_policy())); e.close()
    (ra, xa), la, lra, pa = out[0]; (rb, xb), lb, lrb, pb = out[1]
    assert ra[2:].tobytes() == rb.tobytes() and np.array_equal(xa[2:], xb) and lra[2:].tobytes() == lrb.tobytes()
    for a, b in zip(la + pa, lb + pb):
        assert np.array_equal(a[2:], b)
    assert np.array_equal(lrb["n_stale"], delay[2:])
    sh.close(); s.close()


def test_cpp_latency_loop_matches_the_python_path(hip_lib, tmp_path):
    """tests/cpp/latency_loop.cpp built against libhsddp_hip.so and run for 3 ticks (B = 3, delays 0, 1, 2, the plain walk) through
    hsddp::Episode::set_latency: the rows, the latency rows and the log equal the Python path's (episode.run_mhpc with delay) bit for bit."""
    B, T = 3, 3
    delay = [0, 1, 2]
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    opt0 = first_solve_setting(opt0)
    x0 = ec.start_states(pkg, ph, B)
    exe = tmp_path / "latency_loop"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "latency_loop.cpp"), "-L", os.path.join(ROOT, "cafe-mpc_amd"), "-lhsddp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cafe-mpc_amd"), "-o", str(exe)])
    (tmp_path / "opt.bin").write_bytes(bytes(opt0)); (tmp_path / "x0.bin").write_bytes(x0.tobytes())
    out = json.loads(subprocess.check_output([str(exe), ec.TREE, "bound", str(tmp_path / "opt.bin"), str(tmp_path / "x0.bin"), str(B), str(ec.START_WINDOW), str(T)]
                                             + [str(d) for d in delay], timeout=120))
    s = pkg.MultiPhaseDDP(ph, batch=B)
    e = s.episode(n, T, keep_log=True); e.reset(x0); s.solve(opt0)
    ep.run_mhpc(s, pd, ph, opt_rt, T, episode=e, delay=delay)
    rows, _ = e.rows(); X, U, _ = e.log(); lr = e.latency_rows()
    assert out["n_exec"] == n
    for b in range(B):
        for f, v in out["rows"][b].items():
            assert v == rows[f][b], (b, f, v, rows[f][b])
    assert out["latency"] == [[int(a), int(c)] for a, c in zip(lr["delay"], lr["n_stale"])] and list(lr["n_stale"]) == [0, 2, 4]
    assert np.array_equal(np.array(out["X"]).reshape(X.shape), X) and np.array_equal(np.array(out["U"]).reshape(U.shape), U)
    assert np.abs(U).max() > 0.0
    e.close(); s.close()
