"""GPU tests of the regularised Riccati sweep BY VALUE: k_sweep / k_sweep_hkd / k_sweep32 at reg > 0 against the fp64 oracle, and the in-kernel
retry loop of sweep_body (riccati_sweep again and again on one LDS block and one set of prefetch registers until a factorisation passes), which
no emulator covers.  Plain tolerances (1e-8 x scale per iterate, K 1e-6 absolute, compare_solve's for full solves): no arbiter.  The inputs and
their margins to the accept / reject boundary of the ladder: tests/reg_common.py, pinned on the CPU by test_reg_sweep_host.py."""
import numpy as np
import pytest

from conftest import pkg
import parity_common as pc
import reg_common as rc

pytestmark = pytest.mark.gpu

CASES = [c.name for c in rc.indefinite_cases()]


@pytest.mark.parametrize("which", rc.FIXED_PROBLEMS)
def test_sweep_matches_oracle_at_fixed_reg(hip_lib, oracle_lib, which):
    """k_sweep (whole body, SRB tail) and k_sweep_hkd at reg in (1e-3, 0.4, 37.5): sweep fields, ok flags, DX after the linear rollout and both
    expected cost changes.  Measured on the device: worst error / scale 5.5e-12 and worst |dK| 4.3e-10 (both hkd at reg 1e-3); the whole-body and
    single-rigid-body problems stay below 2.6e-13 and 5.1e-12."""
    phases, x0, opt = rc.fixed_problem(which, batch=3 if which in ("trot", "mhpc") else 2)
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, x0)
    for s in (so, sg):
        rc.prepare(s, opt)
    for reg in rc.REGS:
        oks = [s.backward_sweep(reg) for s in (so, sg)]
        assert oks[0].all() and np.array_equal(oks[0], oks[1])
        rc.compare_sweep(so, sg, len(phases), opt, f"hip {which} reg={reg}")


@pytest.mark.parametrize("name", CASES)
def test_retry_loop_by_value(hip_lib, oracle_lib, name):
    """solve() on inputs whose Quu is indefinite until reg passes -r dt: the in-kernel loop must stop on the rung reg_common computes (the VALUE of
    n_reg_iters, not only equality with the oracle) and leave the sweep of that rung: compare_solve plus G and H0, which SOLVE_FIELDS lacks.  Then
    two DDP iterations: the second search starts from the carried reg / 20."""
    case = rc.case_by_name(name); e = rc.expected_counts(case); nph = len(case.phases())
    so, sg = case.solver(oracle_lib), case.solver(hip_lib)
    o1 = case.opt(max_AL_iter=1, max_DDP_iter=1)
    so.solve(o1); sg.solve(o1)
    ia, ib = so.info_arrays(), sg.info_arrays()
    assert (ib["n_reg_iters"] == e["n_reg_1"]).all() and (ia["n_reg_iters"] == e["n_reg_1"]).all(), (ia["n_reg_iters"], ib["n_reg_iters"], e)
    assert (ib["status"] == 0).all() and (ib["n_iters"] == 1).all()
    rep = pc.compare_solve(so, sg, nph, tag=f"retry {name} 1")
    rep.update(pc.compare(so, sg, ["G", "H0"], nph, 1e-8, f"retry {name} 1"))
    print(f"[reg] retry {name} one iteration: n_reg_iters {ib['n_reg_iters']}, worst error / scale {max(v[0] / v[1] for v in rep.values()):.2e}")
    so.close(); sg.close()
    so, sg = case.solver(oracle_lib), case.solver(hip_lib)
    o2 = case.opt(max_AL_iter=1, max_DDP_iter=2)
    so.solve(o2); sg.solve(o2)
    ia, ib = so.info_arrays(), sg.info_arrays()
    rep = pc.compare_solve(so, sg, nph, tag=f"retry {name} 2")      # counts and status identical to the oracle's
    assert (ib["n_iters"] == 2).all() and (ib["n_reg_iters"] == e["n_reg_2"]).all(), (ib, e)
    print(f"[reg] retry {name} two iterations: n_reg_iters {ib['n_reg_iters']}, n_ls_iters {ib['n_ls_iters']}, worst error / scale {max(v[0] / v[1] for v in rep.values()):.2e}")


@pytest.mark.parametrize("name", ["trot_mid", "hkd"])
def test_rejected_attempt_leaves_no_trace_on_the_device(hip_lib, oracle_lib, name):
    """History independence: a handle that ran the last rejected rung and then the accepted one holds bit-identical sweep fields to a handle that
    only ran the accepted one; both match the oracle.  (trot_mid fails in phase 2 of 4: phase 3's fields are written, phases 1 and 0 are not.)"""
    case = rc.case_by_name(name); e = rc.expected_counts(case); phases = case.phases(); opt = case.opt(); x0 = case.x0(phases)
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, x0)
    so2, fresh = pc.make_pair(pkg, oracle_lib, hip_lib, phases, x0)
    for s in (so, sg, so2, fresh):
        rc.prepare(s, opt)
    for s in (so, sg):
        assert not s.backward_sweep(e["rejected"]).any()
    for s in (so, sg, so2, fresh):
        assert s.backward_sweep(e["accepted"]).all()
    rc.fields_equal(sg, fresh, len(phases))
    rc.compare_sweep(so, sg, len(phases), opt, f"hip {name} rejected -> accepted")
    rc.compare_sweep(so2, fresh, len(phases), opt, f"hip {name} accepted only")
    rc.fields_equal(sg, fresh, len(phases), ["DX"])


def test_give_up_exit(hip_lib, oracle_lib):
    """r = -7000 on the stance problem: critical reg 70, above the last rung 65.536.  An ordinary numerical outcome: status 1 after 18 attempts, one
    iteration, no line search, the nominal trajectory untouched; a well-posed handle created afterwards solves with status 0."""
    case = rc.case_by_name("stance"); phases = case.phases(r=-7000.0)
    so, sg = case.solver(oracle_lib, phases), case.solver(hip_lib, phases)
    o1 = case.opt(max_AL_iter=1, max_DDP_iter=1)
    so.solve(o1); sg.solve(o1)
    ia, ib = so.info_arrays(), sg.info_arrays()
    for i_ in (ia, ib):
        assert (i_["status"] == 1).all() and (i_["n_reg_iters"] == 18).all() and (i_["n_iters"] == 1).all() and (i_["n_ls_iters"] == 0).all(), i_
    rep = pc.compare(so, sg, ["XBAR", "UBAR"], 1, 1e-8, "give-up")
    assert all(np.isfinite(sg.field(0, f)).all() for f in ("XBAR", "UBAR"))
    print(f"[reg] give-up: worst error / scale {max(v[0] / v[1] for v in rep.values()):.2e}")
    so.close(); sg.close()
    good = pkg.problems.wb_stance_problem(horizon=6)
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, good, case.x0(good))
    so.solve(o1); sg.solve(o1)
    assert (sg.info_arrays()["status"] == 0).all() and (sg.info_arrays()["n_reg_iters"] == 1).all()
    pc.compare_solve(so, sg, 1, tag="after give-up")


# per-field relative limits of the fp32 handles: those test_gpu_parity.py holds at reg = 0 on the same problems
# (test_fp32_handle_kinodynamic_parity_with_measured_tolerance: tol, first-iterate record fields 1e-6; test_fp32_handle_single_rigid_body_phases: lim)
F32_HKD = {"A": 1e-6, "B": 1e-6, "LXX": 1e-6, "LUU": 1e-6, "LX": 1e-6, "LU": 1e-6, "QUU": 1e-3, "QUX": 1e-3, "K": 1.5e-3, "DU": 2e-3, "G": 3e-4, "DX": 3e-2, "X": 1e-2, "U": 1e-2}
F32_SRB = {"A": 3e-5, "B": 6e-6, "LXX": 4e-6, "LUU": 1e-6, "K": 1e-4, "DU": 1.2e-4, "DX": 1e-3, "X": 3e-4, "U": 3e-5}


@pytest.mark.parametrize("reg", [1e-3, 0.4])
@pytest.mark.parametrize("which", ["hkd", "srb"])
def test_fp32_sweep_at_fixed_reg(hip_lib, oracle_lib, which, reg):
    """k_sweep32 ((R)reg cast to float, dadd in the fp32 tiles) on one iterate against the fp64 oracle, within the limits the fp32 handles hold at
    reg = 0 (regularisation only improves the conditioning of Quu).  Measured on the device (error / max(1, scale)): HKD at reg 1e-3 K 2.6e-4,
    DU 7.9e-6, QUX 2.2e-5, DX 1.1e-3, at reg 0.4 every field below 1e-6; SRB at reg 1e-3 K 3.2e-6, DU 1.0e-6, DX 6.3e-6, at reg 0.4 below 5e-7."""
    if which == "hkd":
        phases = pkg.problems.hkd_trot_problem(horizons=(10, 10, 10, 10)); x0 = pkg.problems.hkd_ensemble_x0(3, 11, phases)
        opt = pkg.problems.hkd_ddp_setting(); lim = F32_HKD; dv_rtol = 1e-3
    else:
        phases = pkg.problems.mhpc_problem(wb_schedule=(), wb_horizons=(), srb_horizons=(8, 7)); x0 = rc.srb_x0(pkg.problems.wb_ensemble_x0(3, 20241230))
        opt = pkg.mhpc_ddp_setting(); lim = F32_SRB; dv_rtol = 2e-3
    so = pkg.Solver(oracle_lib, phases, batch=3); sg = pkg.Solver(hip_lib, phases, batch=3, precision=pkg.PREC_F32)
    assert hip_lib.hsddp_precision(sg.h) == pkg.PREC_F32
    for s in (so, sg):
        for i, p in enumerate(phases):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(x0)
        s.hybrid_rollout(0.0, opt); s.compute_cost(opt); s.update_nominal_trajectory(); s.LQ_approximation(opt)
        assert s.backward_sweep(reg).all()
    da, db = so.get_exp_cost_change(), sg.get_exp_cost_change()
    for s in (so, sg):
        s.linear_rollout(1.0, opt)
    worst = {}
    for f in lim:
        for i in range(len(phases)):
            a, b = so.field(i, f), sg.field(i, f)
            if a.size:
                worst[f] = max(worst.get(f, 0.0), float(np.abs(a - b).max() / max(1.0, np.abs(a).max())))
    print(f"[reg] fp32 {which} reg={reg}: relative errors {({k: float(f'{v:.2e}') for k, v in worst.items()})}, dV {da[0]} {db[0]} {da[1]} {db[1]}")
    assert np.allclose(da[0], db[0], rtol=dv_rtol, atol=1e-3) and np.allclose(da[1], db[1], rtol=dv_rtol), (da, db)
    assert all(worst[f] <= lim[f] for f in lim), {f: (worst[f], lim[f]) for f in lim if worst[f] > lim[f]}
