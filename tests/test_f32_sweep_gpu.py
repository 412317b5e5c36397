"""GPU tests of k_sweep32 (riccati_sweep / linear_rollout with R = float on v_mfma_f32_16x16x4_f32: its own tile shapes and lane mapping, float DPP quad
sums, fp32 LQ records) against a same-input reference bound: tests/f32_common.py.  The float64 statement of the sweep runs on the records READ BACK FROM
THE fp32 HANDLE, so every comparison sees the sweep arithmetic alone, on any iterate; the bound is COND_FACTOR x the level three float32 realisations of
the same statement reach on those records (never above what the older fp32 tests hold).  The inputs are pinned on the CPU by test_f32_sweep_host.py, with
the lane emulator inside COND_FACTOR / 2."""
import numpy as np
import pytest

from conftest import pkg
import reg_common as rc
import f32_common as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_f32_sweep_within_the_reference_bound(hip_lib, oracle_lib, name):
    """First iterate at reg 0, 1e-3 and 0.4, then reg 0 on the second and third iterate of the step API (hybrid_rollout(1) -> cost -> LQ -> sweep -> linear
    rollout), the reference re-fed the handle's records each time: K, DU, QU, QUU, QUX, G, H0, DX of every (phase, problem) and the four expected cost
    changes.  The measured ratios error / L32 are printed (DESIGN.md section 5 keeps the worst)."""
    ph, x0, opt, old = fc.problem(name)
    s = fc.make(hip_lib, ph, x0, precision=fc.F32)
    assert hip_lib.hsddp_precision(s.h) == fc.F32
    fc.prepare(s, opt)
    for reg in fc.REGS:
        assert s.backward_sweep(reg).all()
        fc.check_bound(s, reg, opt, oracle_lib, old, f"hip {name} reg {reg}")
    for it in (2, 3):
        assert s.backward_sweep(0.0).all(); s.linear_rollout(1.0, opt); fc.next_iterate(s, opt)
        assert s.backward_sweep(0.0).all()
        fc.check_bound(s, 0.0, opt, oracle_lib, old, f"hip {name} iterate {it}")


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_f32_sweep_on_the_state_a_short_solve_leaves(hip_lib, oracle_lib, name):
    """solve() with 2 AL x 2 DDP iterations, then hybrid_rollout(0) / compute_cost / LQ_approximation / backward_sweep(reg) as reg_common.check_margins
    does: the sweep over records that carry updated AL multipliers and barrier parameters."""
    ph, x0, opt, old = fc.problem(name)
    s = fc.make(hip_lib, ph, x0, precision=fc.F32)
    o2 = pkg.problems.hkd_ddp_setting(max_AL_iter=2, max_DDP_iter=2) if name != "srb" else pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=2)
    s.solve(o2)
    assert (s.info_arrays()["status"] == 0).all(), s.info_arrays()
    s.hybrid_rollout(0.0, opt); s.compute_cost(opt); s.LQ_approximation(opt)
    for reg in (0.0, 1e-3):
        assert s.backward_sweep(reg).all()
        fc.check_bound(s, reg, opt, oracle_lib, old, f"hip {name} after solve reg {reg}")


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_f32_records_are_the_rounded_twin(hip_lib, name):
    """First iterate, an fp32 handle against an fp64 handle of the same library: the record fields equal np.float32(twin) bit for bit with exact zeros
    kept, the LQ fields outside the record are bit-identical (f32_common.RECORD_FIELDS / OUTSIDE_FIELDS)."""
    ph, x0, opt, _ = fc.problem(name)
    s32, s64 = fc.make(hip_lib, ph, x0, precision=fc.F32), fc.make(hip_lib, ph, x0)
    fc.prepare(s32, opt); fc.prepare(s64, opt)
    fc.check_records(s32, s64, f"hip {name}")


@pytest.mark.parametrize("name", ["hkd", "srb_only"])
def test_f32_retry_loop_by_value(hip_lib, oracle_lib, name):
    """The in-kernel regularisation retry loop on fp32 handles: n_reg_iters after one and after two DDP iterations equals the rung index computed from the
    ladder (reg_common.expected_counts; the 0.8 x / 1.25 x margins to the rungs are two orders above the fp32 rounding of the critical value), status 0,
    and the sweep the one-iteration solve leaves is within the reference bound at the accepted rung (the records: a second handle at the same first
    iterate, which the solve's sweep ran on)."""
    case = fc.indefinite_case(name); e = rc.expected_counts(case); phases = case.phases(); x0 = case.x0(phases); opt = case.opt()
    old = fc.OLD_HKD if name == "hkd" else fc.OLD_SRB
    s1 = fc.make(hip_lib, phases, x0, precision=fc.F32)
    s1.solve(case.opt(max_AL_iter=1, max_DDP_iter=1))
    ia = s1.info_arrays()
    assert (ia["n_reg_iters"] == e["n_reg_1"]).all() and (ia["status"] == 0).all() and (ia["n_iters"] == 1).all(), (ia, e)
    rec = fc.make(hip_lib, phases, x0, precision=fc.F32)
    fc.prepare(rec, opt)
    fc.check_bound(rec, e["accepted"], opt, oracle_lib, old, f"hip retry {name} reg {e['accepted']}", results_of=s1)
    s1.close(); rec.close()
    s2 = fc.make(hip_lib, phases, x0, precision=fc.F32)
    s2.solve(case.opt(max_AL_iter=1, max_DDP_iter=2))
    ib = s2.info_arrays()
    print(f"[f32] retry {name}: n_reg_iters {ia['n_reg_iters']} / {ib['n_reg_iters']}, n_ls_iters {ib['n_ls_iters']}")
    assert (ib["n_reg_iters"] == e["n_reg_2"]).all() and (ib["status"] == 0).all() and (ib["n_iters"] == 2).all(), (ib, e)


@pytest.mark.parametrize("name", ["hkd", "srb_only"])
def test_f32_rejected_attempt_leaves_no_trace_on_the_device(hip_lib, oracle_lib, name):
    """History independence on an fp32 handle: the last rejected rung, then the accepted one, is bit-identical to the accepted rung alone (sweep fields,
    DX, both expected cost changes), and within the reference bound."""
    case = fc.indefinite_case(name); e = rc.expected_counts(case); phases = case.phases(); x0 = case.x0(phases); opt = case.opt()
    old = fc.OLD_HKD if name == "hkd" else fc.OLD_SRB
    s, fresh = fc.make(hip_lib, phases, x0, precision=fc.F32), fc.make(hip_lib, phases, x0, precision=fc.F32)
    fc.prepare(s, opt); fc.prepare(fresh, opt)
    assert not s.backward_sweep(e["rejected"]).any()
    assert s.backward_sweep(e["accepted"]).all() and fresh.backward_sweep(e["accepted"]).all()
    rc.fields_equal(s, fresh, len(phases))
    for q in (0, 1):
        assert np.array_equal(s.get_exp_cost_change()[q], fresh.get_exp_cost_change()[q])
    fc.check_bound(s, e["accepted"], opt, oracle_lib, old, f"hip {name} rejected -> accepted")
    fresh.linear_rollout(1.0, opt)
    rc.fields_equal(s, fresh, len(phases), ["DX"])
    for q in (0, 1):
        assert np.array_equal(s.get_exp_cost_change()[q], fresh.get_exp_cost_change()[q])
