"""Per-problem cost-weight scales (include/hsddp_weights.h) on the device, through libhsddp_hip.so.  Every test runs under the default programs (lane
quads for the whole-body running knots and the terminal knots behind them) and under HSDDP_QUAD=0 HSDDP_QUAD_TERMINAL=0 (the one-wave programs).

The reference is tests/pw_common.StackedOracle: B single-problem oracle handles whose descriptors carry q * sq_b, r * sr_b, qf * sqf_b.

1. test_parity_on_the_device: the per-iterate cases of tests/test_weights_host.py (qualified there), plain tolerances.
2. test_short_full_solves: trot 4 x 6 knots, B = 17: identical iteration, line-search and regularisation counts, compare_solve at its defaults.
3. test_clear_is_a_handle_that_never_had_scales: bit-identical solve, the launch names of a handle without scales.
4. test_scales_survive_reconfigure: three receding-horizon ticks of the bound gait against the stacked oracle, no allocation once warm.
5. test_scales_and_touchdown_heights: all four combinations against oracle descriptors that carry both.
6. test_episode_with_scales: B = 8, 3 ticks, scales set once, against a hand-written loop of solve + simulate; track_cost with the descriptors' weights.
7. test_abi_and_shards: refusals (fp32 handle included), a device-memory source, the get round trip, a slice of the batch with its slice of rows.

CPU counterpart (lane emulator, ABI, build): tests/test_weights_host.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import episode_common as ec
import parity_common as pc
import pattern_common as pt
import pw_common as pw
import sim_common as sc
import touchdown_common as tdc
from conftest import pkg

pytestmark = pytest.mark.gpu
ep = pkg.episode
EINVAL, ENOTSUP = -1, -4
FIELDS = ["XBAR", "UBAR", "X", "U", "Y", "K", "DU", "QU", "QUU", "QUX", "L", "PHI", "DEFECT"]


@pytest.fixture(params=["default", "wave"])
def programs(request, monkeypatch):
    """The rollout programs of the handles a test creates: the environment is read when a handle is made."""
    for k in ("HSDDP_QUAD", "HSDDP_QUAD_TERMINAL"):
        if request.param == "wave":
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)
    return request.param


def _x0(case, batch):
    return pkg.problems.wb_ensemble_x0(batch, pw.CASES[case][1])


def _snapshot(s):
    ia = s.info_arrays()
    return [s.field(i, f).tobytes() for i in range(len(s.phases)) for f in FIELDS] + [ia[k].tobytes() for k in sorted(ia) if k != "solve_time_ms"]


@pytest.mark.parametrize("batch", pw.BATCHES)
@pytest.mark.parametrize("case", list(pw.CASES))
def test_parity_on_the_device(hip_lib, oracle_lib, programs, case, batch):
    phases = pw.CASES[case][0](); x0 = _x0(case, batch); rows = pw.scale_rows(batch)
    so = pw.StackedOracle(oracle_lib, phases, x0, rows)
    sg = pw.make_hip(hip_lib, phases, x0, rows)
    report = pc.run_steps(pkg, so, sg, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[weights] device {case} B={batch} {programs}: error / tolerance {pt.worst_ratio(report)}")
    names = list(sg.kernel_times())
    assert "k_rollout_pw" in names and "k_lq_pw" in names and "k_rollout" not in names and "k_lq" not in names, names
    so.close(); sg.close()


def test_short_full_solves(hip_lib, oracle_lib, programs):
    B = 17
    phases = pkg.problems.wb_trot_problem(horizons=(6, 6, 6, 6)); x0 = pkg.problems.wb_ensemble_x0(B, pt.SEED); rows = pw.scale_rows(B)
    opt = pt.solve_options()
    so = pw.StackedOracle(oracle_lib, phases, x0, rows); so.solve(opt)
    sg = pw.make_hip(hip_lib, phases, x0, rows); sg.solve(opt)
    ia, ib = so.info_arrays(), sg.info_arrays()
    print(f"[weights] solve {programs}: iterations {ib['n_iters'].tolist()} line-search {ib['n_ls_iters'].tolist()} regularisation {ib['n_reg_iters'].tolist()}")
    report = pc.compare_solve(so, sg, len(phases))
    print(f"[weights] solve {programs}: error / tolerance {pt.worst_ratio(report)}")
    assert len(set(ia["actual_cost"].round(6))) == B      # every robot solved a problem of its own
    so.close(); sg.close()


def test_clear_is_a_handle_that_never_had_scales(hip_lib, programs):
    B = 5
    phases = pw.CASES["flight"][0](); x0 = _x0("flight", B); opt = pt.solve_options()
    never = pw.make_hip(hip_lib, phases, x0); never.solve(opt)
    parent_names = set(never.kernel_times())
    s = pw.make_hip(hip_lib, phases, x0, pw.scale_rows(B))      # set -> clear -> solve (a solve in between would leave its ReB / AL parameters behind)
    s.hybrid_rollout(0.0, opt)
    assert "k_rollout_pw" in s.kernel_times()
    s.clear_weight_scales()
    assert all(np.all(a == 1.0) for a in s.weight_scales())
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    hip_lib.hsddp_reset_kernel_times(s.h)
    s.solve(opt)
    a, b = _snapshot(never), _snapshot(s)
    assert a == b, [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:5]
    names = {n for n, (_, c) in s.kernel_times().items() if c > 0}
    assert names <= parent_names and not any(n.endswith("_pw") for n in names), names
    never.close(); s.close()


class _Both:
    """shift_solver_in_place for the device handle and the stacked oracle with one call to the builder."""

    def __init__(self, *solvers):
        self.solvers = solvers

    def reconfigure(self, phases, src, shift):
        for s in self.solvers:
            s.reconfigure(phases, src, shift)


def _stack_reconfigure(stack, rows):
    def reconfigure(phases, src, shift):
        for b, s in enumerate(stack.s):
            s.reconfigure(pw.scaled_phases(phases, rows[b]), src, shift)
        stack.phases = phases
    stack.reconfigure = reconfigure


def test_scales_survive_reconfigure(hip_lib, oracle_lib, programs):
    """Three receding-horizon ticks of the bound gait (every window of it has 35 knots, a young phase without shooting nodes among them) with the
    scales set ONCE before the first solve; each tick both sides start from the device plan's state one MPC step on, so nothing compounds."""
    B = 3
    pd, phases, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    opt0.max_AL_iter, opt0.max_DDP_iter = 2, 3
    x0 = ec.start_states(pkg, phases, B); rows = pw.scale_rows(B)
    so = pw.StackedOracle(oracle_lib, phases, x0, rows); _stack_reconfigure(so, rows)
    sg = pw.make_hip(hip_lib, phases, x0, rows)
    so.solve(opt0); sg.solve(opt0)
    pc.compare_solve(so, sg, len(phases), tag="first solve")
    mallocs = []
    for tick in range(3):
        xg = sg.field(0, "XBAR")
        x0n = np.ascontiguousarray(xg[:, n] if xg.shape[1] > n else sg.field(1, "XBAR")[:, n - xg.shape[1] + 1])
        phases = ec.shift(pkg, _Both(sg, so), phases, pd)
        assert np.array_equal(np.concatenate(sg.weight_scales(), axis=1), rows)
        sg.set_initial_condition(x0n); so.set_initial_condition(x0n)
        sg.solve(opt_rt); so.solve(opt_rt)
        report = pc.compare_solve(so, sg, len(phases), tag=f"tick {tick}")
        print(f"[weights] reconfigure tick {tick} {programs}: error / tolerance {pt.worst_ratio(report)}")
        mallocs.append(hip_lib.hsddp_debug_malloc_count())
    assert mallocs[1:] == [mallocs[1]] * 2, mallocs
    assert "k_rollout" not in sg.kernel_times() and "k_rollout_pw" in sg.kernel_times()
    so.close(); sg.close()


@pytest.mark.parametrize("scales,heights", [(False, False), (True, False), (False, True), (True, True)])
def test_scales_and_touchdown_heights(hip_lib, oracle_lib, programs, scales, heights):
    B = 5
    phases = pw.CASES["flight"][0](); x0 = _x0("flight", B)
    rows = pw.scale_rows(B) if scales else np.ones((B, pw.ROW))
    td = [i for i, l in enumerate(tdc.td_legs(phases)) if l.any()]
    assert td
    hts = {i: np.repeat(np.round(np.random.default_rng(3 + i).uniform(-0.02, 0.02, size=(B, 1)), 4), 4, axis=1) for i in td} if heights else {}
    so = pw.StackedOracle(oracle_lib, phases, x0, rows, hts)
    sg = pw.make_hip(hip_lib, phases, x0, rows if scales else None)
    for i, h in hts.items():
        sg.set_touchdown_heights(i, h)
    report = pc.run_steps(pkg, so, sg, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[weights] scales {scales} heights {heights} {programs}: error / tolerance {pt.worst_ratio(report)}")
    if scales and heights:      # heights cleared while the scales stay: the scaled terminal programs read the shared value again
        sg.clear_touchdown_heights()
        for i, p in enumerate(phases):
            sg.set_nominal(i, p["Xbar"], p["Ubar"])
        sg.set_initial_condition(x0)
        s2 = pw.StackedOracle(oracle_lib, phases, x0, rows)
        pc.run_steps(pkg, s2, sg, phases, pkg.mhpc_ddp_setting(), n_iter=1)
        s2.close()
    so.close(); sg.close()


def test_episode_with_scales(hip_lib, programs):
    """B = 8, 3 ticks from a window whose first phase has ten knots left (no touchdown falls on a tick boundary).  A: run_mhpc with weight_scales;
    M: set_weight_scales once, then per tick a one-sample Simulation, fold_rows in numpy with the DESCRIPTORS' weights, set_initial_condition."""
    B, T = 8, 3
    pdA, phA, cfg, opt0, opt_rt, n = ec.bound_problem(pkg, 3)
    pdM, phM = ec.bound_problem(pkg, 3)[:2]
    opt0.max_AL_iter, opt0.max_DDP_iter = 3, 4
    x0 = ec.start_states(pkg, phA, B); rows = pw.scale_rows(B)
    A = pkg.MultiPhaseDDP(phA, batch=B); M = pkg.MultiPhaseDDP(phM, batch=B)
    M.set_weight_scales(*pw.split(rows))
    plain = pkg.MultiPhaseDDP(phM, batch=B); plain.set_initial_condition(x0); plain.solve(opt0)
    epi = A.episode(n, T); epi.reset(x0); M.set_initial_condition(x0)
    A.set_weight_scales(*pw.split(rows))      # (run_mhpc sets them again from weight_scales=: the same rows)
    A.solve(opt0); M.solve(opt0)
    assert A.field(0, "K").tobytes() == M.field(0, "K").tobytes() and A.field(0, "K")[1:].tobytes() != plain.field(0, "K")[1:].tobytes()
    plain.close()
    dist = pkg.sim.Disturbance(seed=11, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=20.0)
    state, erows_by_tick, xs_by_tick = x0.copy(), [], []

    def hook(t, phases):
        erows_by_tick.append(epi.rows())
    # A: the library's loop; its rows after each tick's advance are taken by the hook (before that tick's solve)
    res = ep.run_mhpc(A, pdA, phA, opt_rt, T, dist=dist, hook=hook, episode=epi, weight_scales=pw.split(rows))
    mrows = ep.empty_rows(B)
    for t in range(T):
        smap = sc.step_map(phM, n)
        assert ec.pending_phase(phM, n) < 0
        dm = dataclasses.replace(dist, seed=ep.tick_seed(dist.seed, t))
        sim = pkg.Simulation(M, 1, n, keep_traj=True); sim.run(np.ascontiguousarray(state[:, None]), dist=dm)
        srows, xf = sim.rows(); extra = sim.extra(); X, U = sim.traj(); sim.close()
        q, r = ep.step_weights(phM, smap); xr, ur = ep.step_refs(M, smap)      # the descriptors' weights: the yardstick all robots share
        mrows = ep.fold_rows(mrows, t, srows[:, 0], X[:, 0], U[:, 0], q, r, xr, ur, extra=extra[:, 0], status=M.info_arrays()["status"])
        state = xf[:, 0].copy()
        erows, ex = erows_by_tick[t]
        for f in mrows.dtype.names:
            if f != "track_cost":
                assert np.array_equal(erows[f], mrows[f]), (t, f, erows[f], mrows[f])
        rel = np.abs(erows["track_cost"] - mrows["track_cost"]) / np.abs(mrows["track_cost"])
        print(f"[weights] episode tick {t} {programs}: track_cost {erows['track_cost']}, rel diff to the descriptors' weights {rel.max():.3e}")
        assert rel.max() <= 1e-12 and (mrows["end_reason"] == 0).all()
        assert np.array_equal(ex, state)
        M.set_initial_condition(state)
        phM = ec.shift(pkg, M, phM, pdM)
        M.solve(opt_rt)
    for i in range(len(phM)):
        assert A.field(i, "K").tobytes() == M.field(i, "K").tobytes(), i
    assert np.array_equal(np.concatenate(A.weight_scales(), axis=1), rows)
    epi.close(); A.close(); M.close()


def _dev_copy(hip, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def test_abi_and_shards(hip_lib, programs):
    B = 5
    lib = pkg._abi.bind_weights(hip_lib)
    phases = pw.CASES["trot"][0](); x0 = _x0("trot", B); rows = pw.scale_rows(B); opt = pt.solve_options()
    s = pw.make_hip(hip_lib, phases, x0)
    assert all(np.all(a == 1.0) for a in s.weight_scales())
    # first call on a range: the others at 1.0; later calls overwrite their range only; broadcasting from one row
    s.set_weight_scales(*pw.split(rows[1:3]), b0=1)
    want = np.ones((B, pw.ROW)); want[1:3] = rows[1:3]
    assert np.array_equal(np.concatenate(s.weight_scales(), axis=1), want)
    s.set_weight_scales(*pw.split(rows[4:]), b0=4); want[4] = rows[4]
    assert np.array_equal(np.concatenate(s.weight_scales(), axis=1), want) and np.array_equal(np.concatenate(s.weight_scales(2, 3), axis=1), want[2:5])
    s.set_weight_scales(rows[3, :36], rows[3, 36:48], rows[3, 48:], b0=3); want[3:] = rows[3]
    assert np.array_equal(np.concatenate(s.weight_scales(), axis=1), want)
    # refusals leave the handle as it was
    m0 = hip_lib.hsddp_debug_malloc_count(); ok = np.full((B, pw.ROW), 1.5)
    bads = []
    for e, v in ((0, np.nan), (40, 0.0), (40, -1.0), (50, -0.5), (83, np.inf)):
        a = ok.copy(); a[2, e] = v; bads.append(a)
    for args in [(None, 0, B, ok.ctypes.data, 0), (s.h, 0, B, None, 0), (s.h, -1, 2, ok.ctypes.data, 0), (s.h, 0, 0, ok.ctypes.data, 0), (s.h, 1, B, ok.ctypes.data, 0),
                 (s.h, B, 1, ok.ctypes.data, 0)] + [(s.h, 0, B, a.ctypes.data, 0) for a in bads]:
        assert lib.hsddp_weights_set(*args) == EINVAL, args
    assert lib.hsddp_weights_get(s.h, 0, B + 1, ok.ctypes.data) == EINVAL and lib.hsddp_weights_get(s.h, 0, B, None) == EINVAL and lib.hsddp_weights_get(None, 0, B, ok.ctypes.data) == EINVAL
    assert lib.hsddp_weights_clear(None) == EINVAL
    assert np.array_equal(np.concatenate(s.weight_scales(), axis=1), want) and hip_lib.hsddp_debug_malloc_count() == m0
    hk = pkg.problems.hkd_trot_problem()
    k = pkg.Solver(hip_lib, hk, batch=2, precision=pkg.PREC_F32)
    assert lib.hsddp_weights_set(k.h, 0, 2, ok.ctypes.data, 0) == ENOTSUP and lib.hsddp_weights_get(k.h, 0, 2, ok.ctypes.data) == ENOTSUP
    k.close()
    k = pkg.Solver(hip_lib, hk, batch=2)      # a window without a whole-body phase stores the scales and does not use them
    k.set_weight_scales(*pw.split(rows[:2]))
    assert np.array_equal(np.concatenate(k.weight_scales(), axis=1), rows[:2])
    k.close()
    # a device-memory source (the host does not read it), then the solve of the whole batch and of a slice with its slice of rows
    d = _dev_copy(hip_lib, rows)
    assert lib.hsddp_weights_set(s.h, 0, B, d, 1) == 0
    hip_lib.hipFree(d)
    assert np.array_equal(np.concatenate(s.weight_scales(), axis=1), rows)
    s.solve(opt)
    sh = pw.make_hip(hip_lib, phases, np.ascontiguousarray(x0[2:]), rows[2:]); sh.solve(opt)
    for i in range(len(phases)):
        for f in ("K", "XBAR", "UBAR"):
            assert sh.field(i, f).tobytes() == s.field(i, f, 2, 3).tobytes(), (i, f)
    ia, ib = s.info_arrays(), sh.info_arrays()
    for kk in pc.COUNT_KEYS:
        assert np.array_equal(ia[kk][2:], ib[kk]), kk
    s.close(); sh.close()
