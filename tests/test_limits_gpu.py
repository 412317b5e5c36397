"""Per-problem constraint limits (include/hsddp_limits.h) on the device, through libhsddp_hip.so.  Every test runs under the default programs (lane
quads for the whole-body running knots and the terminal knots behind them) and under HSDDP_QUAD=0 HSDDP_QUAD_TERMINAL=0 (the one-wave programs).

The reference is tests/lim_common.LimitedOracle: B single-problem oracle handles whose descriptors carry problem b's limits.

1. test_parity_on_the_device: the per-iterate inputs of tests/test_limits_host.py (qualified and covered there), B = 1, 5, 17, plain tolerances; the
   guard against a run without limits as there.
2. test_short_full_solves: B = 17: identical iteration, line-search and regularisation counts, compare_solve at its defaults.
3. test_clear_is_a_handle_that_never_had_limits: bit-identical solve, the launch names of a handle without limits.
4. test_limits_survive_reconfigure: three receding-horizon ticks of the bound gait with the limits set once; hsddp_limits_get on every window; no
   allocation once warm.
5. test_limits_scales_and_touchdown_heights: all three against oracle descriptors that carry all three.
6. test_limits_without_scales_are_limits_with_unit_scales: bit for bit.
7. test_plan_friction_on_an_episode: the mu column is the numpy product; ticks equal a hand-written loop that calls set_limits.
8. test_abi_and_shards: refusals (fp32 handle included), a device-memory source, first call / later calls, a slice of the batch with its slice of rows.

CPU counterpart (lane emulator, ABI, build): tests/test_limits_host.py."""
import ctypes as C

import numpy as np
import pytest

import episode_common as ec
import lim_common as lc
import parity_common as pc
import pattern_common as pt
import pw_common as pw
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


@pytest.fixture(scope="module")
def inputs(oracle_lib):
    """(phases, x0, rows) at B = 17, as tests/test_limits_host.py builds them; computed once."""
    ph = lc.phases(); x0 = lc.x0_of(17)
    return ph, x0, lc.limit_rows(17, ph, lc.forces(oracle_lib, ph, x0))


def _snapshot(s):
    ia = s.info_arrays()
    return [s.field(i, f).tobytes() for i in range(len(s.phases)) for f in FIELDS] + [ia[k].tobytes() for k in sorted(ia) if k != "solve_time_ms"]


def _renominal(s, phases, x0):
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)


@pytest.mark.parametrize("batch", lc.BATCHES)
def test_parity_on_the_device(hip_lib, oracle_lib, programs, inputs, batch):
    ph, x0, rows = inputs[0], inputs[1][:batch], inputs[2][:batch]
    so = lc.LimitedOracle(oracle_lib, ph, x0, rows)
    sg = lc.make_hip(hip_lib, ph, x0, rows)
    for i in range(len(ph)):
        assert lc.rows_of(sg.limits(i)).tobytes() == lc.resolved(ph, rows)[i].tobytes(), i
    report = pc.run_steps(pkg, so, sg, ph, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[limits] device B={batch} {programs}: error / tolerance {pt.worst_ratio(report)}")
    names = list(sg.kernel_times())
    assert "k_rollout_lim" in names and "k_lq_lim" in names and not {"k_rollout", "k_lq", "k_rollout_pw", "k_lq_pw"} & set(names), names
    sn = lc.make_hip(hip_lib, ph, x0); s0 = lc.LimitedOracle(oracle_lib, ph, x0, np.full_like(rows, np.nan))      # the guard: no limits
    pc.run_steps(pkg, s0, sn, ph, pkg.mhpc_ddp_setting(), n_iter=2)
    for b in range(1, batch):
        ratio = max(np.abs(sg.field(i, f)[b] - sn.field(i, f)[b]).max() / (1e-8 * max(1.0, np.abs(sg.field(i, f)).max())) for f in ("LX", "LU") for i in range(len(ph)))
        assert ratio > 100.0, (b, ratio)
    for s in (so, sg, sn, s0):
        s.close()


def test_short_full_solves(hip_lib, oracle_lib, programs, inputs):
    ph, x0, rows = inputs
    opt = pt.solve_options()
    so = lc.LimitedOracle(oracle_lib, ph, x0, rows); so.solve(opt)
    sg = lc.make_hip(hip_lib, ph, x0, rows); sg.solve(opt)
    ib = sg.info_arrays()
    print(f"[limits] solve {programs}: iterations {ib['n_iters'].tolist()} line-search {ib['n_ls_iters'].tolist()} regularisation {ib['n_reg_iters'].tolist()}")
    report = pc.compare_solve(so, sg, len(ph))
    print(f"[limits] solve {programs}: error / tolerance {pt.worst_ratio(report)}")
    names = {n for n, (_, c) in sg.kernel_times().items() if c > 0}
    assert {"k_rollout_lim", "k_lq_lim", "k_ls_probe_lim"} <= names and not {"k_rollout", "k_lq", "k_ls_probe"} & names, names
    so.close(); sg.close()


def test_clear_is_a_handle_that_never_had_limits(hip_lib, programs, inputs):
    ph, x0, rows = inputs[0], inputs[1][:5], inputs[2][:5]
    opt = pt.solve_options()
    never = lc.make_hip(hip_lib, ph, x0); never.solve(opt)
    parent_names = set(never.kernel_times())
    s = lc.make_hip(hip_lib, ph, x0, rows)      # set -> clear -> solve (a solve in between would leave its ReB / AL parameters behind)
    s.hybrid_rollout(0.0, opt)
    assert "k_rollout_lim" in s.kernel_times()
    s.clear_limits()
    for i in range(len(ph)):
        assert lc.rows_of(s.limits(i)).tobytes() == np.tile(lc.desc_row(ph[i]["desc"]), (5, 1)).tobytes()
    _renominal(s, ph, x0)
    hip_lib.hsddp_reset_kernel_times(s.h)
    s.solve(opt)
    a, b = _snapshot(never), _snapshot(s)
    assert a == b, [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:5]
    names = {n for n, (_, c) in s.kernel_times().items() if c > 0}
    assert names <= parent_names and not any(n.endswith("_lim") or n.endswith("_pw") for n in names), names
    never.close(); s.close()


class _Both:
    """shift_solver_in_place for the device handle and the stacked oracle with one call to the builder."""

    def __init__(self, *solvers):
        self.solvers = solvers

    def reconfigure(self, phases, src, shift):
        for s in self.solvers:
            s.reconfigure(phases, src, shift)


def test_limits_survive_reconfigure(hip_lib, oracle_lib, programs):
    """Three receding-horizon ticks of the bound gait with the limits set ONCE before the first solve; each tick both sides start from the device
    plan's state one MPC step on, so nothing compounds."""
    B = 3
    pd, phases, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    opt0.max_AL_iter, opt0.max_DDP_iter = 2, 3
    x0 = ec.start_states(pkg, phases, B); rows = lc.simple_rows(B)
    so = lc.LimitedOracle(oracle_lib, phases, x0, rows)
    sg = lc.make_hip(hip_lib, phases, x0, rows)
    so.solve(opt0); sg.solve(opt0)
    pc.compare_solve(so, sg, len(phases), tag="first solve")
    mallocs = []
    for tick in range(3):
        xg = sg.field(0, "XBAR")
        x0n = np.ascontiguousarray(xg[:, n] if xg.shape[1] > n else sg.field(1, "XBAR")[:, n - xg.shape[1] + 1])
        phases = ec.shift(pkg, _Both(sg, so), phases, pd)
        res = lc.resolved(phases, rows)
        for i, p in enumerate(phases):      # the rows against the NEW window's descriptors, reduced-model phases included (stored, unused)
            assert lc.rows_of(sg.limits(i)).tobytes() == res[i].tobytes(), (tick, i)
        sg.set_initial_condition(x0n); so.set_initial_condition(x0n)
        sg.solve(opt_rt); so.solve(opt_rt)
        report = pc.compare_solve(so, sg, len(phases), tag=f"tick {tick}")
        print(f"[limits] reconfigure tick {tick} {programs}: error / tolerance {pt.worst_ratio(report)}")
        mallocs.append(hip_lib.hsddp_debug_malloc_count())
    assert mallocs[1:] == [mallocs[1]] * 2, mallocs
    assert "k_rollout" not in sg.kernel_times() and "k_rollout_lim" in sg.kernel_times() and "k_pack_limits" in sg.kernel_times()
    so.close(); sg.close()


def test_limits_scales_and_touchdown_heights(hip_lib, oracle_lib, programs):
    B = 5
    phases = pw.CASES["flight"][0](); x0 = pkg.problems.wb_ensemble_x0(B, pw.CASES["flight"][1])
    rows = lc.simple_rows(B); scales = pw.scale_rows(B)
    td = [i for i, l in enumerate(tdc.td_legs(phases)) if l.any()]
    assert td
    hts = {i: np.repeat(np.round(np.random.default_rng(3 + i).uniform(-0.02, 0.02, size=(B, 1)), 4), 4, axis=1) for i in td}
    so = lc.LimitedOracle(oracle_lib, phases, x0, rows, scales, hts)
    sg = lc.make_hip(hip_lib, phases, x0, rows, scales)
    for i, h in hts.items():
        sg.set_touchdown_heights(i, h)
    report = pc.run_steps(pkg, so, sg, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[limits] limits x scales x heights {programs}: error / tolerance {pt.worst_ratio(report)}")
    # heights and scales cleared while the limits stay: the kernels with limits read the shared height and ones again
    sg.clear_touchdown_heights(); sg.clear_weight_scales(); _renominal(sg, phases, x0)
    s2 = lc.LimitedOracle(oracle_lib, phases, x0, rows)
    pc.run_steps(pkg, s2, sg, phases, pkg.mhpc_ddp_setting(), n_iter=1)
    assert "k_rollout_lim" in sg.kernel_times()
    for s in (so, sg, s2):
        s.close()


def test_limits_without_scales_are_limits_with_unit_scales(hip_lib, programs, inputs):
    ph, x0, rows = inputs[0], inputs[1][:5], inputs[2][:5]
    opt = pt.solve_options()
    a = lc.make_hip(hip_lib, ph, x0, rows); a.solve(opt)
    b = lc.make_hip(hip_lib, ph, x0, rows, np.ones((5, pw.ROW))); b.solve(opt)
    assert all(np.all(w == 1.0) for w in a.weight_scales())      # the ones the kernels read are not the handle's scale table: none is set
    sa, sb = _snapshot(a), _snapshot(b)
    assert sa == sb, [k for k, (x, y) in enumerate(zip(sa, sb)) if x != y][:5]
    a.close(); b.close()


def test_plan_friction_on_an_episode(hip_lib, programs):
    """B = 6 robots on three grounds, two ticks.  A: Episode.plan_friction(kappa) once; M: Solver.set_limits(mu = kappa * mu_s[mu_of]) from numpy.
    The mu column equals the product bit for bit, the other entries stay, and both sides' plans agree bit for bit on every tick."""
    B, T, kappa = 6, 2, 0.7
    pdA, phA, cfg, opt0, opt_rt, n = ec.bound_problem(pkg, 3)
    pdM, phM = ec.bound_problem(pkg, 3)[:2]
    opt0.max_AL_iter, opt0.max_DDP_iter = 2, 3
    x0 = ec.start_states(pkg, phA, B)
    mu_tab = np.array([[0.6, 0.5], [0.25, 0.2], [0.3, 0.3]]); mu_of = np.array([0, 1, 2, 2, 1, 0], dtype=np.int32)
    fr = pkg.sim.Friction(mu=mu_tab, mu_of=mu_of[:, None], v_stick=0.02)
    A = pkg.MultiPhaseDDP(phA, batch=B); M = pkg.MultiPhaseDDP(phM, batch=B)
    lim = pkg._abi.bind_limits(hip_lib)
    epi = A.episode(n, T); epi.reset(x0)
    assert lim.hsddp_episode_plan_friction(epi.e, kappa) == EINVAL      # no friction set
    epi.set_contact(-3.0, 0.0); epi.set_friction(fr)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        assert lim.hsddp_episode_plan_friction(epi.e, bad) == EINVAL, bad
    assert lim.hsddp_episode_plan_friction(None, kappa) == EINVAL
    A.set_limits(torque_limit=np.linspace(10.0, 15.0, B)); M.set_limits(torque_limit=np.linspace(10.0, 15.0, B))
    epi.plan_friction(kappa)
    want = kappa * mu_tab[mu_of, 0]
    for i in range(len(phA)):
        got = A.limits(i)
        assert got["mu"].tobytes() == want.tobytes() and np.array_equal(got["torque_limit"], np.linspace(10.0, 15.0, B)), i
        assert np.array_equal(got["h_min"], np.full(B, phA[i]["desc"].h_min))
    M.set_limits(torque_limit=np.linspace(10.0, 15.0, B), mu=want)      # (set_limits writes whole rows: the torque limits go in again)
    A.set_initial_condition(x0); M.set_initial_condition(x0)
    A.solve(opt0); M.solve(opt0)
    assert A.field(0, "K").tobytes() == M.field(0, "K").tobytes()
    state = x0
    for t in range(T):
        epi.advance()
        state = epi.rows()[1]
        phA = ec.shift(pkg, A, phA, pdA); phM = ec.shift(pkg, M, phM, pdM)
        assert A.limits(0)["mu"].tobytes() == want.tobytes()      # set once: the rows stay across the tick's reconfigure
        M.set_initial_condition(state)
        A.solve(opt_rt); M.solve(opt_rt)
        for i in range(len(phA)):
            for f in ("K", "XBAR", "UBAR"):
                assert A.field(i, f).tobytes() == M.field(i, f).tobytes(), (t, i, f)
    assert "k_lim_mu" in A.kernel_times() and "k_lq_lim" in A.kernel_times()
    # a handle without a table: plan_friction makes one with every other entry unset
    A.clear_limits(); epi.plan_friction(1.0)
    got = A.limits(0)
    assert got["mu"].tobytes() == mu_tab[mu_of, 0].tobytes() and np.array_equal(got["torque_limit"], np.full(B, phA[0]["desc"].torque_limit))
    epi.close(); A.close(); M.close()


def _dev_copy(hip, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def test_abi_and_shards(hip_lib, programs, inputs):
    B = 5
    lib = pkg._abi.bind_limits(hip_lib)
    ph, x0, rows = inputs[0], inputs[1][:B], inputs[2][:B]
    opt = pt.solve_options()
    s = lc.make_hip(hip_lib, ph, x0)
    drow = [np.tile(lc.desc_row(p["desc"]), (B, 1)) for p in ph]
    assert all(lc.rows_of(s.limits(i)).tobytes() == drow[i].tobytes() for i in range(len(ph)))      # no table: the descriptors' values
    # first call on a range: the others unset; later calls overwrite their range only; scalars broadcast
    s.set_limits(**lc.row_kwargs(rows[1:3]), b0=1)
    want = np.full((B, lc.ROW), np.nan); want[1:3] = rows[1:3]
    assert lc.rows_of(s.limits(1)).tobytes() == lc.resolved(ph, want)[1].tobytes()
    s.set_limits(**lc.row_kwargs(rows[4:]), b0=4); want[4] = rows[4]
    assert lc.rows_of(s.limits(0)).tobytes() == lc.resolved(ph, want)[0].tobytes() and lc.rows_of(s.limits(2, 2, 3)).tobytes() == lc.resolved(ph, want)[2][2:5].tobytes()
    s.set_limits(mu=0.35, torque_limit=11.0, b0=3); want[3:] = np.nan; want[3:, lc.MU] = 0.35; want[3:, lc.TORQUE] = 11.0
    assert lc.rows_of(s.limits(0)).tobytes() == lc.resolved(ph, want)[0].tobytes()
    # refusals leave the handle as it was
    m0 = hip_lib.hsddp_debug_malloc_count()
    ok = np.tile(np.array([12.0, -0.3, -1.2, 1.8, 0.3, -0.8, 2.2, 0.1, 0.4, -3.0, 3.0, np.nan]), (B, 1))
    bads = []
    for e, v in ((lc.TORQUE, 0.0), (lc.MU, -0.1), (lc.JLB, 0.5), (lc.JSUB, -4.0), (lc.HMIN, np.inf)):
        a = ok.copy(); a[2, e] = v; bads.append(a)
    for args in [(None, 0, B, ok.ctypes.data, 0), (s.h, 0, B, None, 0), (s.h, -1, 2, ok.ctypes.data, 0), (s.h, 0, 0, ok.ctypes.data, 0), (s.h, 1, B, ok.ctypes.data, 0),
                 (s.h, B, 1, ok.ctypes.data, 0)] + [(s.h, 0, B, a.ctypes.data, 0) for a in bads]:
        assert lib.hsddp_limits_set(*args) == EINVAL, args
    for args in ((s.h, 0, 0, B + 1, ok.ctypes.data), (s.h, 0, 0, B, None), (None, 0, 0, B, ok.ctypes.data), (s.h, len(ph), 0, B, ok.ctypes.data), (s.h, -1, 0, B, ok.ctypes.data)):
        assert lib.hsddp_limits_get(*args) == EINVAL, args
    assert lib.hsddp_limits_clear(None) == EINVAL
    assert lc.rows_of(s.limits(0)).tobytes() == lc.resolved(ph, want)[0].tobytes() and hip_lib.hsddp_debug_malloc_count() == m0
    hk = pkg.problems.hkd_trot_problem()
    k = pkg.Solver(hip_lib, hk, batch=2, precision=pkg.PREC_F32)
    assert lib.hsddp_limits_set(k.h, 0, 2, ok.ctypes.data, 0) == ENOTSUP and lib.hsddp_limits_get(k.h, 0, 0, 2, ok.ctypes.data) == ENOTSUP and lib.hsddp_limits_clear(k.h) == ENOTSUP
    k.close()
    k = pkg.Solver(hip_lib, hk, batch=2)      # a window without a whole-body phase stores the rows and does not use them
    k.set_limits(mu=np.array([0.3, 0.4]))
    assert np.array_equal(k.limits(0)["mu"], [0.3, 0.4]) and np.array_equal(k.limits(0)["torque_limit"], np.full(2, hk[0]["desc"].torque_limit))
    k.hybrid_rollout(0.0, pkg.mhpc_ddp_setting())
    assert not any(n.endswith("_lim") for n in k.kernel_times())
    k.close()
    # a device-memory source (the host does not read it), then the solve of the whole batch and of a slice with its slice of rows
    d = _dev_copy(hip_lib, np.ascontiguousarray(rows))
    assert lib.hsddp_limits_set(s.h, 0, B, d, 1) == 0
    hip_lib.hipFree(d)
    for i in range(len(ph)):
        assert lc.rows_of(s.limits(i)).tobytes() == lc.resolved(ph, rows)[i].tobytes()
    s.solve(opt)
    sh = lc.make_hip(hip_lib, ph, np.ascontiguousarray(x0[2:]), rows[2:]); sh.solve(opt)
    for i in range(len(ph)):
        for f in ("K", "XBAR", "UBAR"):
            assert sh.field(i, f).tobytes() == s.field(i, f, 2, 3).tobytes(), (i, f)
    ia, ib = s.info_arrays(), sh.info_arrays()
    for kk in pc.COUNT_KEYS:
        assert np.array_equal(ia[kk][2:], ib[kk]), kk
    s.close(); sh.close()
