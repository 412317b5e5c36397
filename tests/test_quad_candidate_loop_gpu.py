"""The lane-quad rollout kernel evaluates the candidates of a probe launch one after the other in the same wave, its step-independent inputs staged
in LDS once per unit (16 problems x one knot).  That is a schedule, not a result: however the ladder of a line search is cut into probe launches
(HSDDP_LS_CHUNK), and wherever the full step is rolled out (HSDDP_LS_SPECULATE), the solves end bit-identical - and the quad program still agrees
with the one-wave program (HSDDP_QUAD=0), which has no candidate loop and reads every input from global memory.

The three shapes were run on the CPU oracle: every problem ends with status 0 and the line-search counts per problem are spread (12-84, 14-41,
32-104), so probe launches run with partial problem lists and searches accept at mixed positions of the ladder.
"""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

FIELDS = ("XBAR", "UBAR", "K", "DU", "X", "U")
HANDLES = tuple((chunk, spec) for chunk in ("1", "3", None) for spec in ("0", "1"))      # (HSDDP_LS_CHUNK, HSDDP_LS_SPECULATE)


def _solve(monkeypatch, phases, x0, opt, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    s = pkg.MultiPhaseDDP(phases, batch=x0.shape[0])
    s.set_initial_condition(x0); s.solve(opt)
    return s


def _assert_schedules_are_invisible(monkeypatch, phases, x0, opt):
    """One handle per (chunk, speculate); every info field and XBAR, UBAR, K, DU, X, U of every phase bit-identical to the first handle's."""
    sols = {(chunk, spec): _solve(monkeypatch, phases, x0, opt, {"HSDDP_LS_CHUNK": chunk, "HSDDP_LS_SPECULATE": spec}) for chunk, spec in HANDLES}
    first = sols[HANDLES[0]]
    ia = first.info_arrays()
    assert (ia["status"] == 0).all()
    assert (ia["n_ls_iters"] > ia["n_iters"]).any()      # probe launches happened
    for key in HANDLES[1:]:
        io = sols[key].info_arrays()
        for k in ia:
            assert np.array_equal(ia[k], io[k]), (key, k)
        for ph in range(len(phases)):
            for f in FIELDS:
                assert np.array_equal(first.field(ph, f), sols[key].field(ph, f)), (key, ph, f)
    return sols


def test_loop_of_n_candidates_equals_n_launches_of_one(hip_lib, monkeypatch):
    """HSDDP_LS_CHUNK=1 makes every probe launch a one-trip loop: anything a wave carried from one candidate to the next (a register, a staged row
    overwritten, the writer flag) would show as a difference against the handles whose launches loop over three candidates or the whole ladder.
    17 problems = one full wave and a single quad; in the one-knot phases knot 0 is also the last running knot, and phase 0 has the x0 defect."""
    phases = pkg.problems.wb_trot_problem(horizons=(3, 1, 2, 1))
    x0 = pkg.problems.wb_ensemble_x0(17, 20241220 + 3)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=12, cost_thresh=0.0)
    _assert_schedules_are_invisible(monkeypatch, phases, x0, opt)


def test_partial_lists_and_commits(hip_lib, monkeypatch):
    """A hard start (zero torques): searches accept in the middle of the ladder, so later chunks run on the list of problems still searching (any
    length, not a multiple of 16) and accepted probes are followed by commit launches (one-trip loops with the problem's own step length)."""
    phases = pkg.problems.wb_stance_problem(horizon=6, ubar_mode="zero")
    x0 = np.vstack([pkg.problems.wb_nominal_state()[None], pkg.problems.wb_ensemble_x0(20, 7)])
    opt = pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=6, cost_thresh=0.0)
    sols = _assert_schedules_are_invisible(monkeypatch, phases, x0, opt)
    for spec in ("0", "1"):
        assert sols[("3", spec)].kernel_times()["k_ls_probe"][1] > sols[(None, spec)].kernel_times()["k_ls_probe"][1]      # the chunked handle really launched more probe kernels


def test_candidate_loop_against_the_one_wave_program(hip_lib, monkeypatch):
    """The criterion of test_quad_and_one_wave_rollout_programs_agree on a fixed-work solve that walks whole ladders: counts and status equal, cost
    to 1e-9 relative, trajectories and gains to 1e-8 of their scale."""
    phases = pkg.problems.wb_trot_problem(horizons=(20, 20, 20, 20))
    x0 = pkg.problems.wb_ensemble_x0(17, 20241220 + 3)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=14, cost_thresh=0.0)
    a, b = (_solve(monkeypatch, phases, x0, opt, {"HSDDP_QUAD": flag}) for flag in ("1", "0"))
    ia, ib = a.info_arrays(), b.info_arrays()
    for k in ("n_iters", "n_ls_iters", "n_reg_iters", "status"):
        assert np.array_equal(ia[k], ib[k]), k
    assert (ia["status"] == 0).all()
    assert (ia["n_ls_iters"] > ia["n_iters"]).any()      # probe launches happened
    assert np.allclose(ia["actual_cost"], ib["actual_cost"], rtol=1e-9)
    for i in range(len(phases)):
        for f in ("XBAR", "UBAR", "K", "Y"):
            fa, fb = a.field(i, f), b.field(i, f)
            assert np.abs(fa - fb).max() <= 1e-8 * max(1.0, np.abs(fa).max()), (i, f, np.abs(fa - fb).max())
