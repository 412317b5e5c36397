"""CPU tests of the regularised Riccati sweep (reg > 0) BY VALUE: the oracle against a numpy restatement, the kernel program sweep.hpp (lane
emulator tests/_emu) against the oracle at fixed reg, a rejected attempt followed by the accepted one on the same handle, and the margins of
the indefinite inputs the device tests of the retry loop lean on (tests/reg_common.py).  Plain tolerances throughout (1e-8 x scale, K 1e-6
absolute): no arbiter."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import parity_common as pc
import reg_common as rc
from test_oracle_solver import numpy_backward_sweep


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "_emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    return pkg._abi.bind(ctypes.CDLL(os.path.join(d, "libhsddp_emu.so")))


def _one_phase(which):
    if which == "wb":        # 36 / 12 / 12
        return pkg.problems.wb_stance_problem(horizon=10), pkg.problems.wb_ensemble_x0(1, 3)
    ph = pkg.problems.mhpc_problem(wb_schedule=(), wb_horizons=(), srb_schedule=((1, 0, 0, 1),), srb_horizons=(6,))      # 12 / 12 / 0
    return ph, rc.srb_x0(pkg.problems.wb_ensemble_x0(1, 3))


@pytest.fixture(scope="module")
def one_phase_oracle(oracle_lib):
    """One prepared oracle handle per model and its reg = 0 sweep results (computed once, left unchanged)."""
    out = {}
    for which in ("wb", "srb"):
        ph, x0 = _one_phase(which)
        s = pc.make_pair(pkg, oracle_lib, oracle_lib, ph, x0)[0]
        rc.prepare(s, pkg.mhpc_ddp_setting())
        assert s.backward_sweep(0.0).all()
        out[which] = (s, s.field(0, "QUU")[0].copy(), s.field(0, "H0")[0, 0].copy())
    return out


@pytest.mark.parametrize("reg", rc.REGS)
@pytest.mark.parametrize("which", ["wb", "srb"])
def test_oracle_sweep_against_numpy_at_positive_reg(one_phase_oracle, which, reg):
    """The oracle's own +reg (SinglePhase.cpp:364-365): gains, feed-forward and expected cost change against numpy at the limits of
    test_riccati_against_numpy, the stored Quu and H[0] by value, and what the reference keeps: Quu is stored WITH reg, and reg sits on Qxx too
    (quirk x), so H[0] moves on its diagonal."""
    s, quu0, h00 = one_phase_oracle[which]
    n, m, p = s.dims[0]
    assert s.backward_sweep(reg).all()
    Ks, dUs, dV, Quus, H0 = rc.numpy_sweep(s, reg)
    K, DU, QUU, H = s.field(0, "K")[0], s.field(0, "DU")[0], s.field(0, "QUU")[0], s.field(0, "H0")[0, 0]
    dV1, dV2 = s.get_exp_cost_change()
    print(f"[reg] oracle vs numpy {which} reg {reg}: dK {np.abs(K - Ks).max():.2e} dDU {np.abs(DU - dUs).max():.2e} dQuu {np.abs(QUU - Quus).max():.2e} dH0 {np.abs(H - H0).max():.2e}")
    assert np.abs(K - Ks).max() < 1e-8
    assert np.abs(DU - dUs).max() < 1e-9
    assert abs(dV1[0] - dV) < 1e-9 * max(1, abs(dV)) and abs(dV2[0] + dV) < 1e-9 * max(1, abs(dV))
    assert np.abs(QUU - Quus).max() <= 1e-8 * max(1.0, np.abs(Quus).max())
    assert np.abs(H - H0).max() <= 1e-8 * max(1.0, np.abs(H0).max())
    if which == "wb":        # the restatement test_oracle_solver.py holds the oracle to at reg = 0, now with its reg argument in use
        Ko, dUo, dVo = numpy_backward_sweep(s, 1, reg)
        assert np.abs(K - Ko).max() < 1e-8 and np.abs(DU - dUo).max() < 1e-9 and abs(dV1[0] - dVo) < 1e-9 * max(1, abs(dVo))
    # stored Quu = luu + B^T H B + D^T lyy D + reg I, and H grows with reg: every diagonal entry gains at least reg, the last knot's exactly reg
    gain = np.diagonal(QUU - quu0, axis1=1, axis2=2)
    slack = 1e-12 * max(1.0, np.abs(quu0).max())
    assert (gain >= reg - slack).all(), gain.min()
    assert np.abs(gain[-1] - reg).max() <= slack
    assert (np.diagonal(H - h00) >= reg - 1e-12 * max(1.0, np.abs(h00).max())).all(), np.diagonal(H - h00).min()


@pytest.mark.parametrize("which", rc.FIXED_PROBLEMS)
def test_emulated_sweep_matches_oracle_at_fixed_reg(emu_lib, oracle_lib, which):
    """sweep.hpp (riccati_sweep, sweep_tiles2's dadd on the diagonal Qxx / Quu tiles, linear_rollout) against the oracle at reg > 0 on every phase
    shape: 36/12/12 with its 4-wide edge tile, 12/12/0, 24/24/0, mixed dimensions across an impact, a four-foot touchdown, one-knot phases,
    single shooting."""
    phases, x0, opt = rc.fixed_problem(which)
    so, se = pc.make_pair(pkg, oracle_lib, emu_lib, phases, x0)
    for s in (so, se):
        rc.prepare(s, opt)
    for reg in rc.REGS:
        oks = [s.backward_sweep(reg) for s in (so, se)]
        assert oks[0].all() and np.array_equal(oks[0], oks[1])
        rc.compare_sweep(so, se, len(phases), opt, f"emu {which} reg={reg}")


@pytest.mark.parametrize("name", [c.name for c in rc.indefinite_cases()])
def test_rejected_then_accepted_sweep_on_one_handle(emu_lib, oracle_lib, name):
    """The last rejected rung, then the accepted one, on the same handles: the rejected attempt leaves partly written fields (and, in the emulator
    as on the device, its H / Quu / prefetch state in the LDS block), none of which may reach the accepted result.  The emulator handle that
    failed first is bit-identical to a fresh one that only ran the accepted sweep."""
    case = rc.case_by_name(name); phases = case.phases(); opt = case.opt(); x0 = case.x0(phases)
    e = rc.expected_counts(case)
    so, se = pc.make_pair(pkg, oracle_lib, emu_lib, phases, x0)
    fresh = pc.make_pair(pkg, emu_lib, emu_lib, phases, x0)[0]
    for s in (so, se, fresh):
        rc.prepare(s, opt)
    for s in (so, se):
        assert not s.backward_sweep(e["rejected"]).any()
    for s in (so, se, fresh):
        assert s.backward_sweep(e["accepted"]).all()
    rc.compare_sweep(so, se, len(phases), opt, f"emu {name} rejected {e['rejected']} -> accepted {e['accepted']}")
    fresh.linear_rollout(1.0, opt)
    rc.fields_equal(se, fresh, len(phases), rc.SWEEP_FIELDS + ["DX"])
    for q in (0, 1):
        assert np.array_equal(se.get_exp_cost_change()[q], fresh.get_exp_cost_change()[q])


@pytest.mark.parametrize("name", [c.name for c in rc.indefinite_cases()])
def test_indefinite_inputs_sit_clear_of_the_ladder_rungs(oracle_lib, oracle_ld_lib, name):
    """check_margins (a condition on the inputs), the counts the device tests expect, and the identity the device test of the retry loop leans
    on: the sweep fields a one-iteration solve leaves are bit-identical to backward_sweep(accepted reg) through the step API."""
    case = rc.case_by_name(name)
    m = rc.check_margins(case, oracle_lib, oracle_ld_lib)
    e = rc.expected_counts(case)
    print(f"[reg] {name}: {m}")
    assert all(m[k] == e[k] for k in e), (m, e)
    s1, s2, s3 = case.solver(oracle_lib), case.solver(oracle_lib), case.solver(oracle_lib)
    s1.solve(case.opt(max_AL_iter=1, max_DDP_iter=1))
    rc.prepare(s2, case.opt())
    assert abs(rc.critical_reg(s2, 0) - m["critical"][0]) <= 1e-7 * m["critical"][0]      # the one-problem bisection agrees with the joint one
    assert s2.backward_sweep(m["accepted"]).all()
    rc.fields_equal(s1, s2, len(s1.phases))
    s3.solve(case.opt(max_AL_iter=1, max_DDP_iter=2))
    i1, i3 = s1.info_arrays(), s3.info_arrays()
    assert (i1["n_reg_iters"] == m["n_reg_1"]).all() and (i3["n_reg_iters"] == m["n_reg_2"]).all() and (i3["n_iters"] == 2).all(), (i1, i3)


def test_ladder_and_give_up_count():
    opt = pkg.mhpc_ddp_setting()
    lad = rc.ladder(opt)
    assert lad[:3] == [0.0, 1e-3, 2e-3] and len(lad) == 18 and abs(lad[-1] - 65.536) < 1e-12        # a search that gives up has tried 18 values
    assert rc.ladder(opt, 0.0256)[:2] == [0.0256, 0.0512] and rc.ladder(opt, 2e-4)[:3] == [2e-4, 1e-3, 2e-3]
    assert rc.carried(0.512) == 0.0256 and rc.carried(1e-5) == 0.0


def test_give_up_exit_on_the_oracle(oracle_lib):
    """r = -7000: critical reg 70, above the last rung 65.536.  The search gives up: status 1 after 18 attempts, no line search, finite trajectories."""
    case = rc.case_by_name("stance")
    s = case.solver(oracle_lib, case.phases(r=-7000.0))
    s.solve(case.opt(max_AL_iter=1, max_DDP_iter=1))
    ia = s.info_arrays()
    assert (ia["status"] == 1).all() and (ia["n_reg_iters"] == 18).all() and (ia["n_iters"] == 1).all() and (ia["n_ls_iters"] == 0).all(), ia
    assert np.isfinite(s.field(0, "XBAR")).all() and np.isfinite(s.field(0, "UBAR")).all()
