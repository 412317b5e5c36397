"""GPU tests of per-problem touchdown heights and terrain-aware planning (include/hsddp_touchdown.h).

1. Oracle parity with heights uniform per problem: one batch-5 handle against five batch-1 oracle solves whose descriptors carry the height as
   ground_height on every phase; per-iterate (parity_common.run_steps) and full solve (compare_solve) at their default tolerances, identical counts.
2. Heights by leg (a, b, b, a): in this gait phases 1 and 3 land legs 0, 3 and phase 2 lands legs 1, 2, so the oracle states it with per-phase
   ground_height a, b, a.  Pins the leg indexing.
3. Different heights inside one touchdown (no oracle for it): the th rule and the Phi rule of the CPU test through hsddp_touchdown_get and the PHI,
   AL_SIGMA, AL_LAMBDA fields; max_tconstr; the one-wave variant (HSDDP_QUAD_TERMINAL=0) against the quad variant; a young phase without shooting
   nodes (the chain of k_rollout_tdh) against the oracle.
4. Dormancy and lifetime.   5. hsddp_touchdown_from_terrain against the numpy definition.   6. Closed loop on a curb."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import parity_common as pc
import episode_common as ec
import touchdown_common as tdc

pytestmark = pytest.mark.gpu

SEED = 20241222
EINVAL, ENOTSUP = -1, -4
ALL_FIELDS = [f for f in pkg._abi.FIELDS]


class Stack:
    """Batch-1 solvers side by side behind the calls parity_common makes of one solver."""

    def __init__(self, solvers):
        self.s = solvers; self.batch = len(solvers); self.phases = solvers[0].phases

    def field(self, i, f):
        return np.concatenate([s.field(i, f) for s in self.s])

    def info_arrays(self):
        d = [s.info_arrays() for s in self.s]
        return {k: np.concatenate([x[k] for x in d]) for k in d[0]}

    def measure_dynamics_feasibility(self):
        return np.concatenate([s.measure_dynamics_feasibility() for s in self.s])

    def backward_sweep(self, reg):
        return np.concatenate([s.backward_sweep(reg) for s in self.s])

    def get_exp_cost_change(self):
        a = [s.get_exp_cost_change() for s in self.s]
        return tuple(np.concatenate([x[q] for x in a]) for q in (0, 1))

    def __getattr__(self, name):
        return lambda *a, **k: [getattr(s, name)(*a, **k) for s in self.s]


def _nominal(s, phases):
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    return s


def _oracle_uniform(oracle_lib, make, x0, heights):
    """One batch-1 oracle solver per problem, ground_height = the problem's height on every phase."""
    out = []
    for b, g in enumerate(heights):
        ph = make()
        for p in ph:
            p["desc"].ground_height = float(g)
        s = _nominal(pkg.Solver(oracle_lib, ph, batch=1), ph); s.set_initial_condition(x0[b:b + 1]); out.append(s)
    return Stack(out)


def _gpu(hip_lib, phases, x0, heights=None):
    """heights: [B, 4] for every phase with a touchdown, or {phase: [B, 4]}."""
    s = _nominal(pkg.Solver(hip_lib, phases, batch=x0.shape[0]), phases); s.set_initial_condition(x0)
    legs = tdc.td_legs(phases)
    if heights is not None:
        for i in range(len(phases)):
            if legs[i].any():
                s.set_touchdown_heights(i, heights[i] if isinstance(heights, dict) else heights)
    return s


UNIFORM = np.array([0.0, 0.03, -0.02, 0.05, 0.01])


def _parity(hip_lib, make_oracle, phases, x0, heights, tag):
    opt = pkg.mhpc_ddp_setting()
    sa, sb = make_oracle(), _gpu(hip_lib, phases, x0, heights)
    pc.run_steps(pkg, sa, sb, phases, opt, n_iter=2)
    sa.close(); sb.close()
    opt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4)
    sa, sb = make_oracle(), _gpu(hip_lib, phases, x0, heights)
    sa.solve(opt); sb.solve(opt)
    ia = sa.info_arrays()
    print(f"[touchdown] {tag}: oracle status {ia['status'].tolist()} iterations {ia['n_iters'].tolist()}")
    assert (ia["status"] == 0).all()
    pc.compare_solve(sa, sb, len(phases), tag=tag)
    sa.close(); sb.close()
    return ia


def test_oracle_parity_heights_uniform_per_problem(hip_lib, oracle_lib):
    make = lambda: pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    phases = make()
    x0 = pkg.problems.wb_ensemble_x0(5, SEED)
    ia = _parity(hip_lib, lambda: _oracle_uniform(oracle_lib, make, x0, UNIFORM), phases, x0, np.repeat(UNIFORM[:, None], 4, axis=1), "uniform heights")
    assert len(set(ia["n_iters"].tolist())) > 1      # the heights change the solves: a build that ignores them cannot match all five


def test_oracle_parity_heights_by_leg(hip_lib, oracle_lib):
    a, b = 0.03, -0.02
    make = lambda: pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    phases = make()
    legs = tdc.td_legs(phases)
    assert legs.tolist() == [[False] * 4, [True, False, False, True], [False, True, True, False], [True, False, False, True]]
    x0 = pkg.problems.wb_ensemble_x0(5, SEED)

    def oracle():
        ph = make()
        for p, g in zip(ph, (0.0, a, b, a)):
            p["desc"].ground_height = g
        s = _nominal(pkg.Solver(oracle_lib, ph, batch=5), ph); s.set_initial_condition(x0)
        return s
    _parity(hip_lib, oracle, phases, x0, np.tile(np.array([a, b, b, a]), (5, 1)), "heights by leg")


def _mixed_case(batch):
    phases = pkg.problems.wb_trot_problem(horizons=(3, 1, 2, 1))
    x0 = pkg.problems.wb_ensemble_x0(batch, SEED)
    hts = tdc.mixed_heights(batch, len(phases))
    return phases, x0, {i: hts[:, i] for i in range(len(phases))}


def test_different_heights_inside_one_touchdown(hip_lib):
    """Batch 17: one wave of the quad kernel is partly filled."""
    B = 17
    phases, x0, hts = _mixed_case(B)
    legs = tdc.td_legs(phases)
    opt = pkg.mhpc_ddp_setting()
    s0, sh = _gpu(hip_lib, phases, x0), _gpu(hip_lib, phases, x0, hts)
    s0.hybrid_rollout(0.0, opt); sh.hybrid_rollout(0.0, opt)
    worst = np.zeros(B)
    for i in range(len(phases)):
        if not legs[i].any():
            assert hip_lib.hsddp_touchdown_get(sh.h, i, 0, B, None, None) == EINVAL      # no touchdown constraint
            continue
        h0, v0 = s0.touchdown(i); hh, vh = sh.touchdown(i)
        assert np.array_equal(h0, np.zeros((B, 4))) and np.array_equal(hh, hts[i])
        assert np.isnan(v0[:, ~legs[i]]).all() and np.isnan(vh[:, ~legs[i]]).all() and not np.isnan(vh[:, legs[i]]).any()
        assert np.array_equal(vh[:, legs[i]], v0[:, legs[i]] - hts[i][:, legs[i]]), (i, "th is not th0 - height bit for bit")
        nt = int(legs[i].sum())
        sg, lm = sh.field(i, "AL_SIGMA").reshape(B, nt), sh.field(i, "AL_LAMBDA").reshape(B, nt)
        assert np.array_equal(sg, s0.field(i, "AL_SIGMA").reshape(B, nt))
        p0, ph_ = s0.field(i, "PHI").reshape(B), sh.field(i, "PHI").reshape(B)
        d = (ph_ - p0) - (tdc.al_sum(vh[:, legs[i]], sg, lm, nt) - tdc.al_sum(v0[:, legs[i]], sg, lm, nt))      # Phibase is the same in both handles
        assert np.abs(d).max() <= 1e-13 * max(1.0, np.abs(ph_).max()), (i, np.abs(d).max())
        assert np.abs(ph_ - p0).max() > 1e-6
        worst = np.maximum(worst, np.abs(vh[:, legs[i]]).max(axis=1))
    # max_tconstr of get_info: the float the history buffer holds after the initial rollout of a solve (no iterations)
    sh.solve(pkg.mhpc_ddp_setting(max_AL_iter=0))
    assert np.array_equal(np.float32(sh.info_arrays()["max_tconstr"]), np.float32(worst))
    s0.close(); sh.close()


def test_one_wave_variant_agrees_with_the_quad_variant(hip_lib, monkeypatch):
    """HSDDP_QUAD_TERMINAL=0 (k_rollout_tdh for every terminal knot) against the default handle (k_rollout_quad_term_tdh) over a 3-iteration solve,
    within the bounds of tests/test_quad_terminal_gpu.py."""
    B = 17
    phases, x0, hts = _mixed_case(B)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=3, cost_thresh=0.0)
    sols = []
    for flag in (None, "0"):
        if flag is None:
            monkeypatch.delenv("HSDDP_QUAD_TERMINAL", raising=False)
        else:
            monkeypatch.setenv("HSDDP_QUAD_TERMINAL", flag)
        s = _gpu(hip_lib, phases, x0, hts); s.solve(opt); sols.append(s)
    monkeypatch.delenv("HSDDP_QUAD_TERMINAL", raising=False)
    a, b = sols
    ia, ib = a.info_arrays(), b.info_arrays()
    for k in ("n_iters", "n_ls_iters", "n_reg_iters", "status"):
        assert np.array_equal(ia[k], ib[k]), (k, ia[k], ib[k])
    assert (ia["n_iters"] == 3).all()
    assert np.allclose(ia["actual_cost"], ib["actual_cost"], rtol=1e-9)
    for i in range(len(phases)):
        for f in ("XBAR", "UBAR", "K", "Y"):
            fa, fb = a.field(i, f), b.field(i, f)
            assert np.abs(fa - fb).max() <= 1e-8 * max(1.0, np.abs(fa).max()), (i, f, np.abs(fa - fb).max())
        if tdc.td_legs(phases)[i].any():
            assert np.array_equal(a.touchdown(i)[0], b.touchdown(i)[0])
    ka, kb = a.kernel_times(), b.kernel_times()
    print("[touchdown] kernels of the default handle", sorted(ka), "of the one-wave handle", sorted(kb))
    a.close(); b.close()


def test_young_phase_chain_against_the_oracle(hip_lib, oracle_lib):
    """Phase 2 without shooting nodes: the terminal wave of phase 1 walks it (rollout_chain in k_rollout_tdh), its terminal knot included."""
    def make():
        ph = pkg.problems.wb_trot_problem(horizons=(3, 2, 2, 3))
        ph[2]["desc"].shooting = 0
        return ph
    phases = make()
    heights = UNIFORM[1:4]
    x0 = pkg.problems.wb_ensemble_x0(3, SEED)
    sa, sb = _oracle_uniform(oracle_lib, make, x0, heights), _gpu(hip_lib, phases, x0, np.repeat(heights[:, None], 4, axis=1))
    pc.run_steps(pkg, sa, sb, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    v = sb.touchdown(2)[1]
    assert not np.isnan(v[:, tdc.td_legs(phases)[2]]).any()
    plain = _gpu(hip_lib, phases, x0); plain.hybrid_rollout(0.0, pkg.mhpc_ddp_setting())      # the heights reached the chain's terminal knot
    sb.hybrid_rollout(0.0, pkg.mhpc_ddp_setting())
    assert np.abs(sb.field(2, "PHI") - plain.field(2, "PHI"))[1:].min() > 1e-6
    sa.close(); sb.close(); plain.close()


def _snapshot(s):
    ia = s.info_arrays()
    return [s.field(i, f).tobytes() for i in range(len(s.phases)) for f in ALL_FIELDS] + [ia[k].tobytes() for k in sorted(ia) if k != "solve_time_ms"]


def test_dormancy_and_lifetime(hip_lib):
    B = 5
    phases, x0, hts = _mixed_case(B)
    nph = len(phases)
    legs = tdc.td_legs(phases)
    td = [i for i in range(nph) if legs[i].any()]
    opt = pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3)
    never = _gpu(hip_lib, phases, x0); never.solve(opt)
    # set -> clear -> solve: bit-identical in every field and in info; one phase at a time and all at once
    for how in ("all", "each"):
        s = _gpu(hip_lib, phases, x0, hts)
        if how == "all":
            s.clear_touchdown_heights()
        else:
            for i in td:
                s.clear_touchdown_heights(i)
        for i in td:
            assert np.array_equal(s.touchdown(i)[0], np.zeros((B, 4)))
        s.solve(opt)
        a, b = _snapshot(never), _snapshot(s)
        assert a == b, [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:5]
        s.close()
    # a phase cleared while another keeps its heights reads the shared value
    s = _gpu(hip_lib, phases, x0, hts); s.clear_touchdown_heights(td[0])
    assert np.array_equal(s.touchdown(td[0])[0], np.zeros((B, 4))) and np.array_equal(s.touchdown(td[1])[0], hts[td[1]])
    one = _gpu(hip_lib, phases, x0, {i: (hts[i] if i != td[0] else np.zeros((B, 4))) for i in range(nph)})
    s.solve(opt); one.solve(opt)
    assert _snapshot(s) == _snapshot(one)
    s.close(); one.close()
    # heights equal to the shared value: the _tdh kernels, the same solve
    s = _gpu(hip_lib, phases, x0, np.zeros((B, 4))); s.solve(opt)
    ia, ib = never.info_arrays(), s.info_arrays()
    for k in ("n_iters", "n_ls_iters", "n_reg_iters", "status"):
        assert np.array_equal(ia[k], ib[k]), k
    for i in range(nph):
        for f in ALL_FIELDS:
            fa, fb = never.field(i, f), s.field(i, f)
            if fa.size:
                assert np.abs(fa - fb).max() <= 1e-12 * max(1.0, np.abs(fa).max()), (i, f, np.abs(fa - fb).max())
    # partial range: the other problems start from the shared value
    s.set_touchdown_heights(td[0], hts[td[0]][1:3], b0=1)
    want = np.zeros((B, 4)); want[1:3] = hts[td[0]][1:3]
    assert np.array_equal(s.touchdown(td[0])[0], want) and np.array_equal(s.touchdown(td[0], 2, 2)[0], want[2:4])
    # hsddp_set_references keeps the heights; hsddp_reconfigure returns to the shared value
    refs = s.get_references(td[0])
    s.set_references(td[0], xr=refs["xr"] + 0.001)
    assert np.array_equal(s.touchdown(td[0])[0], want)
    ident = (list(range(nph)), [0] * nph)
    s.reconfigure(phases, *ident)
    for i in td:
        assert np.array_equal(s.touchdown(i)[0], np.zeros((B, 4)))
    # no device allocation over three warm reconfigure -> set -> solve ticks
    rt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    mallocs = []
    for tick in range(5):
        s.reconfigure(phases, *ident)
        for i in td:
            s.set_touchdown_heights(i, hts[i])
        s.set_initial_condition(x0); s.solve(rt)
        mallocs.append(hip_lib.hsddp_debug_malloc_count())
    assert mallocs[2:] == [mallocs[2]] * 3, mallocs
    # refusals leave the handle as it was
    lib = pkg._abi.bind_touchdown(hip_lib)
    before = [s.touchdown(i)[0].tobytes() for i in td]; m0 = hip_lib.hsddp_debug_malloc_count()
    ok = np.zeros((B, 4)); bad = ok.copy(); bad[2, 1] = np.nan
    no_td = [i for i in range(nph) if not legs[i].any()][0]
    for args in ((None, td[0], 0, B, ok.ctypes.data, 0), (s.h, -1, 0, B, ok.ctypes.data, 0), (s.h, nph, 0, B, ok.ctypes.data, 0), (s.h, td[0], -1, 2, ok.ctypes.data, 0),
                 (s.h, td[0], 0, 0, ok.ctypes.data, 0), (s.h, td[0], 1, B, ok.ctypes.data, 0), (s.h, td[0], 0, B, None, 0), (s.h, td[0], 0, B, bad.ctypes.data, 0),
                 (s.h, no_td, 0, B, ok.ctypes.data, 0)):
        assert lib.hsddp_touchdown_set(*args) == EINVAL, args
    assert lib.hsddp_touchdown_clear(s.h, nph) == EINVAL and lib.hsddp_touchdown_clear(None, 0) == EINVAL and lib.hsddp_touchdown_clear(s.h, -2) == EINVAL
    assert lib.hsddp_touchdown_get(s.h, td[0], 0, B + 1, None, None) == EINVAL
    t = pkg.sim.Terrain(np.zeros((2, 2))).to_c()
    assert lib.hsddp_touchdown_from_terrain(s.h, C.byref(t), None, None, 0.0, 0) == EINVAL and lib.hsddp_touchdown_from_terrain(s.h, None, ok.ctypes.data, None, 0.0, 0) == EINVAL
    assert lib.hsddp_touchdown_from_terrain(s.h, C.byref(t), ok.ctypes.data, None, np.nan, 0) == EINVAL
    assert [s.touchdown(i)[0].tobytes() for i in td] == before and hip_lib.hsddp_debug_malloc_count() == m0
    e = s.episode(2, 2)
    assert lib.hsddp_episode_plan_terrain(e.e) == EINVAL and lib.hsddp_episode_plan_terrain(None) == EINVAL      # no terrain set
    e.close()
    # phases of the other models and fp32 handles keep the shared value
    hk = pkg.problems.hkd_trot_problem()
    k = pkg.Solver(hip_lib, hk, batch=2)
    assert lib.hsddp_touchdown_set(k.h, 0, 0, 2, ok.ctypes.data, 0) == ENOTSUP
    k.close()
    k = pkg.Solver(hip_lib, hk, batch=2, precision=pkg.PREC_F32)
    assert lib.hsddp_touchdown_set(k.h, 0, 0, 2, ok.ctypes.data, 0) == ENOTSUP
    k.close()
    s.close(); never.close()


def _dev_copy(hip, a):
    """A copy of `a` in device memory.  hip: the package's library - looked up through it, hipMalloc / hipMemcpy are those of the HIP runtime the
    library itself is linked against, whatever else the process has loaded."""
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


@pytest.mark.parametrize("use_map", [True, False])
def test_from_terrain_on_the_device_equals_the_numpy_definition(hip_lib, use_map):
    """Inputs of the CPU test: 3 maps of 5 x 4 cells, B = 17; phase 0 with per-problem references, phase 1 with shared ones, phase 2 without a
    touchdown.  Grid and map_of from host memory and from device memory."""
    B = 17
    phases = pkg.problems.wb_trot_problem(schedule=((1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1)), horizons=(2, 3, 2), last_next=(1, 1, 1, 1))
    phases[1]["bufs"]["foot_pos"][:] = tdc.lookup_footholds(1, 4, 6)[0]
    s = pkg.Solver(hip_lib, phases, batch=B)
    s.set_references(0, foot_pos=tdc.lookup_footholds(B, 3, 5))
    ter, mo = tdc.lookup_terrain(), (tdc.lookup_map(B) if use_map else None)
    want = pkg.problems.touchdown_heights_from_terrain(s, ter, mo, 0.0125)
    assert sorted(want) == [0, 1] and len({float(x) for x in want[0].ravel()}) > 10
    s.plan_terrain(ter, mo, 0.0125)
    for i in (0, 1):
        assert np.array_equal(s.touchdown(i)[0], want[i]), ("host", i)
    s.clear_touchdown_heights()
    hip = hip_lib
    dH = _dev_copy(hip, ter.grid()); dM = _dev_copy(hip, mo) if use_map else None
    lib = pkg._abi.bind_touchdown(hip_lib)
    t = ter.to_c()
    assert lib.hsddp_touchdown_from_terrain(s.h, C.byref(t), dH, dM, 0.0125, 1) == 0
    for i in (0, 1):
        assert np.array_equal(s.touchdown(i)[0], want[i]), ("device", i)
    assert hip_lib.hsddp_touchdown_get(s.h, 2, 0, B, None, None) == EINVAL
    s.close()
    for p in (dH, dM):
        if p is not None:
            hip.hipFree(p)


def _curb(B, mo, step):
    """The bound gait from window 11, B start states, and the curb: map 0 steps up by `step` 0.25 m ahead of the trunk, on a cell boundary - the front
    feet stand before it (their footholds of this gait are 0.19 to 0.23 m ahead) and their next reference footholds (0.27 m ahead) lie on it;
    map 1 is flat."""
    pd, ph, cfg, opt0, opt_rt, n = ec.bound_problem(pkg)
    x0 = ec.start_states(pkg, ph, B)
    H = np.zeros((2, 1, 64)); xs = x0[0, 0] + 0.25 + 0.05 * (np.arange(64) - 32)
    H[0, 0, 32:] = step
    ter = pkg.sim.Terrain(H, x0=float(xs[0]), y0=-1.0, cx=0.05, cy=2.0, early=True, w_td=0.0, map_of=mo)
    return pd, ph, opt0, opt_rt, n, x0, ter


def test_closed_loop_on_a_curb(hip_lib):
    """run_mhpc on the bound gait with a curb (map 0: a 0.04 m step ahead of the robots; map 1: flat), contact rule and terrain on, 4 ticks, B = 4,
    with and without terrain-aware planning.  n_early, max_pen and the tracking cost of both runs are printed, not asserted."""
    B, T, STEP = 4, 4, 0.04
    mo = np.array([[0], [1], [0], [1]], dtype=np.int32)
    curb = mo[:, 0] == 0
    results = {}
    for plan in (True, False):
        pd, ph, opt0, opt_rt, n, x0, ter = _curb(B, mo, STEP)
        s = pkg.MultiPhaseDDP(ph, batch=B)
        e = s.episode(n, T); e.set_substeps(2); e.set_contact(0.0, 0.0); e.set_terrain(ter); e.reset(x0); s.solve(opt0)
        seen = dict(n_early=[], max_pen=[], raised=0)

        def after(t, phases):
            legs = tdc.td_legs(phases)
            want = pkg.problems.touchdown_heights_from_terrain(s, ter, mo[:, 0], 0.0)
            ia = s.info_arrays()
            worst = np.zeros(B)
            for i in range(len(phases)):
                if not legs[i].any():
                    continue
                hts, val = s.touchdown(i)
                if plan:
                    assert np.array_equal(hts, want[i]), (t, i)
                    seen["raised"] += int((hts[curb] > 0).any())
                    worst = np.maximum(worst, np.abs(val[:, legs[i]]).max(axis=1))
                else:
                    assert np.array_equal(hts, np.full((B, 4), phases[i]["desc"].ground_height)), (t, i)
                    # the same stored values measured against the terrain: off by the step height where the reference foothold is on the step
                    v, w = val[:, legs[i]], want[i][:, legs[i]]
                    on_step = w > 0
                    assert (w[on_step] == STEP).all() and not on_step[~curb].any()
                    seen["raised"] += int(on_step.any())
                    bound = np.maximum(np.abs(v).max(axis=1), np.float64(ia["max_tconstr"]))[:, None] * np.ones_like(v)
                    assert (np.abs(np.abs(v - w) - STEP)[on_step] <= bound[on_step] + 1e-15).all(), (t, i)
            okb = ia["status"] == 0
            print(f"[touchdown] plan={plan} tick {t}: status {ia['status'].tolist()} max_tconstr {ia['max_tconstr'].tolist()} max|values| {worst.tolist()}")
            if plan:
                assert np.array_equal(np.float32(worst[okb]), np.float32(ia["max_tconstr"][okb])), (t, worst, ia["max_tconstr"])
            tr = e.terrain_rows()
            seen["n_early"].append(tr["n_early"].ravel().tolist()); seen["max_pen"].append(tr["max_pen"].ravel().tolist())
        res = pkg.episode.run_mhpc(s, pd, ph, opt_rt, T, episode=e, plan_terrain=plan, post_hook=after)
        rows, x = e.rows()
        print(f"[touchdown] plan_terrain={plan}: n_early per tick {seen['n_early']}, max_pen per tick {seen['max_pen']}, cost per tick {res['cost'].tolist()}, "
              f"alive {res['alive'].tolist()}, end_reason {rows['end_reason'].tolist()}")
        assert seen["raised"] > 0, "no window of the episode had a reference foothold on the step"
        results[plan] = res
        e.close(); s.close()
    assert results[True]["cost"].shape == results[False]["cost"].shape == (T, B)


def test_cpp_touchdown_loop_matches_the_python_path(hip_lib, tmp_path):
    """tests/cpp/touchdown_loop.cpp built against libhsddp_hip.so and run for 4 ticks on the curb (B = 4, S = 2, the contact rule and the terrain on,
    Episode::plan_terrain every tick): per-tick iterations, costs, alive counts and the touchdown heights in use equal the Python path's
    (episode.run_mhpc(..., plan_terrain=True))."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    B, T, STEP = 4, 4, 0.04
    mo = np.array([[0], [1], [0], [1]], dtype=np.int32)
    pd, ph, opt0, opt_rt, n, x0, ter = _curb(B, mo, STEP)
    exe = tmp_path / "touchdown_loop"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "touchdown_loop.cpp"), "-L", os.path.join(ROOT, "cafe-mpc_amd"), "-lhsddp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cafe-mpc_amd"), "-o", str(exe)])
    H = ter.grid()
    (tmp_path / "opt.bin").write_bytes(bytes(opt0)); (tmp_path / "x0.bin").write_bytes(x0.tobytes())
    (tmp_path / "H.bin").write_bytes(H.tobytes()); (tmp_path / "map.bin").write_bytes(np.ascontiguousarray(mo[:, 0]).tobytes())
    out = json.loads(subprocess.check_output([str(exe), ec.TREE, "bound", str(tmp_path / "opt.bin"), str(tmp_path / "x0.bin"), str(B), str(ec.START_WINDOW), str(T), "2",
                                              str(tmp_path / "H.bin"), str(H.shape[2]), str(H.shape[1]), str(H.shape[0]), repr(ter.x0), repr(ter.y0), repr(ter.cx), repr(ter.cy),
                                              str(tmp_path / "map.bin"), "1"], timeout=120))
    s = pkg.MultiPhaseDDP(ph, batch=B)
    e = s.episode(n, T); e.set_substeps(2); e.set_contact(0.0, 0.0); e.set_terrain(ter); e.reset(x0); s.solve(opt0)
    heights = []

    def after(t, phases):
        td = [i for i in range(len(phases)) if tdc.td_legs(phases)[i].any()]
        heights.append((td[-1], s.touchdown(td[-1])[0].ravel().tolist()) if td else (-1, []))
    res = pkg.episode.run_mhpc(s, pd, ph, opt_rt, T, episode=e, plan_terrain=True, post_hook=after)
    assert out["n_exec"] == n and [t["iters"] for t in out["per_tick"]] == res["n_iters"].tolist() and [t["alive"] for t in out["per_tick"]] == res["alive"].tolist()
    assert np.allclose([t["cost"] for t in out["per_tick"]], res["cost"], rtol=1e-9)
    assert [(t["td_phase"], t["heights"]) for t in out["per_tick"]] == heights
    assert any(STEP in hts for _, hts in heights)
    e.close(); s.close()
