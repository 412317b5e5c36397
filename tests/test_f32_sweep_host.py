"""CPU tests of the fp32 sweep (riccati_sweep / linear_rollout with R = float, the program of k_sweep32) on fp32 handles of the lane emulator, against a
same-input reference bound (tests/f32_common.py): the numpy statement pinned against the oracle, the emulated fp32 sweep within COND_FACTOR / 2 of the
float32 level of every field on the records it was given (first iterate at three reg values, second and third iterate), the fp32 records bit for bit, and
the inputs of the device tests of the fp32 retry loop."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import parity_common as pc
import reg_common as rc
import f32_common as fc


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "_emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    return pkg._abi.bind(ctypes.CDLL(os.path.join(d, "libhsddp_emu.so")))


def _pin(so, reg, opt, px_lib, tag):
    """The oracle's fields after backward_sweep(reg) + linear_rollout(1) against the float64 statement (all three realisations) on the oracle's records."""
    assert so.backward_sweep(reg).all()
    got, gdv = fc.handle_results(so, opt)
    worst = 0.0
    for b in range(so.batch):
        inp = fc.read_inputs(so, b, px_lib)
        for how in fc.REALISATIONS:
            f64, d64 = fc.reference(inp, reg, np.float64, how)
            e = max([fc._err(got[f][i][b], f64[f][i]) for f in fc.FIELDS for i in range(len(inp))] + [fc._rel(gdv[k][b], d64[k]) for k in fc.DV_KEYS])
            worst = max(worst, e)
    print(f"[f32] oracle vs numpy {tag} reg {reg}: worst error / scale {worst:.2e}")
    assert worst <= 1e-10, (tag, reg, worst)       # the level test_riccati_against_numpy holds; measured <= 4.6e-12


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_numpy_statement_reproduces_the_oracle(oracle_lib, name):
    """numpy_sweep_multi / numpy_linear_multi in float64 on the ORACLE's records reproduce the oracle: K, DU, QU, QUU, QUX, G, H0, DX and the four
    expected cost changes at 1e-10 of scale, on every problem at every reg and on every iterate the fp32 tests use - and with each of the three
    realisations, so the hand-written LDLT and the reversed contractions are pinned before they serve as yardsticks."""
    ph, x0, opt, _ = fc.problem(name)
    so = fc.make(oracle_lib, ph, x0); fc.prepare(so, opt)
    for reg in fc.REGS:
        _pin(so, reg, opt, oracle_lib, name)
    for it in (2, 3):
        assert so.backward_sweep(0.0).all(); so.linear_rollout(1.0, opt); fc.next_iterate(so, opt)
        _pin(so, 0.0, opt, oracle_lib, f"{name} iterate {it}")


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_numpy_statement_on_the_state_a_short_solve_leaves(oracle_lib, name):
    """The same pin on the records of the device test that follows a 2 AL x 2 DDP solve (updated AL multipliers and barrier parameters, states off the
    reference, so Px is taken at a moved X[h]): the emulator has no solve, the oracle has."""
    ph, x0, opt, _ = fc.problem(name)
    so = fc.make(oracle_lib, ph, x0)
    so.solve(pkg.problems.hkd_ddp_setting(max_AL_iter=2, max_DDP_iter=2) if name != "srb" else pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=2))
    assert (so.info_arrays()["status"] == 0).all()
    so.hybrid_rollout(0.0, opt); so.compute_cost(opt); so.LQ_approximation(opt)
    for reg in (0.0, 1e-3):
        _pin(so, reg, opt, oracle_lib, f"{name} after solve")


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_emulated_f32_sweep_within_the_reference_bound(emu_lib, oracle_lib, name):
    """The fp32 sweep program on its own records: every field of every (phase, problem) within COND_FACTOR x L32 (check_bound), and - the condition on
    the INPUTS that leaves the device room - every measured ratio error / L32 <= COND_FACTOR / 2.  Measured (worst over the five sweeps of a problem):
    hkd dV_2 after the linear rollout 3.2, hkd_short DX 3.4, srb G 2.5.  If a problem stops meeting the condition, change its seed (f32_common.SEEDS),
    never the factor."""
    ph, x0, opt, old = fc.problem(name)
    s = fc.make(emu_lib, ph, x0, precision=fc.F32)
    assert emu_lib.hsddp_precision(s.h) == fc.F32
    fc.prepare(s, opt)
    ratios = {}
    for reg in fc.REGS:
        assert s.backward_sweep(reg).all()
        ratios[f"reg {reg}"] = fc.check_bound(s, reg, opt, oracle_lib, old, f"emu {name} reg {reg}")
    for it in (2, 3):      # the sweep of a later iterate, on the records of THAT iterate: the reference is re-fed the handle's records
        assert s.backward_sweep(0.0).all(); s.linear_rollout(1.0, opt); fc.next_iterate(s, opt)
        assert s.backward_sweep(0.0).all()
        ratios[f"iterate {it}"] = fc.check_bound(s, 0.0, opt, oracle_lib, old, f"emu {name} iterate {it}")
    over = {(c, k): v for c, r in ratios.items() for k, v in r.items() if k != "share" and v > pc.COND_FACTOR / 2}
    assert not over, f"{name}: the input leaves the device no room: {over}"


@pytest.mark.parametrize("name", fc.PROBLEMS)
def test_emulated_f32_records_are_the_rounded_twin(emu_lib, name):
    """First iterate: every field the fp32 record stores equals np.float32(fp64 twin) bit for bit, exact zeros stay exact zeros, every LQ field kept
    outside the record is bit-identical (lists: f32_common.RECORD_FIELDS / OUTSIDE_FIELDS, from RecLayout and rec_put)."""
    ph, x0, opt, _ = fc.problem(name)
    s32, s64 = fc.make(emu_lib, ph, x0, precision=fc.F32), fc.make(emu_lib, ph, x0)
    fc.prepare(s32, opt); fc.prepare(s64, opt)
    fc.check_records(s32, s64, f"emu {name}")


def test_srb_indefinite_case_sits_clear_of_the_ladder_rungs(oracle_lib, oracle_ld_lib):
    """The new single-rigid-body indefinite input of the fp32 retry-loop tests: check_margins as for reg_common's cases, and the counts from the ladder."""
    case = fc.srb_indefinite_case()
    m = rc.check_margins(case, oracle_lib, oracle_ld_lib)
    e = rc.expected_counts(case)
    print(f"[f32] {case.name}: {m}")
    assert all(m[k] == e[k] for k in e), (m, e)
    assert abs(m["critical"][0] - 0.003) < 3e-6 and (e["rejected"], e["accepted"], e["n_reg_1"]) == (0.002, 0.004, 4)


@pytest.mark.parametrize("name", ["hkd", "srb_only"])
def test_emulated_f32_sweep_on_indefinite_inputs(emu_lib, oracle_lib, name):
    """What the device tests of the fp32 retry loop lean on, with the emulator: the float64 statement reproduces the oracle at the accepted rung; an
    fp32 handle rejects the rung below the critical value and accepts the one above; a handle that ran the rejected rung first is bit-identical to a
    fresh one; the sweep at the accepted rung is within the bound with the ratios <= COND_FACTOR / 2."""
    case = fc.indefinite_case(name); e = rc.expected_counts(case); phases = case.phases(); opt = case.opt(); x0 = case.x0(phases)
    old = fc.OLD_HKD if name == "hkd" else fc.OLD_SRB
    so = fc.make(oracle_lib, phases, x0); fc.prepare(so, opt)
    _pin(so, e["accepted"], opt, oracle_lib, f"indefinite {name}")
    s, fresh = fc.make(emu_lib, phases, x0, precision=fc.F32), fc.make(emu_lib, phases, x0, precision=fc.F32)
    fc.prepare(s, opt); fc.prepare(fresh, opt)
    assert not s.backward_sweep(e["rejected"]).any()
    assert s.backward_sweep(e["accepted"]).all() and fresh.backward_sweep(e["accepted"]).all()
    rc.fields_equal(s, fresh, len(phases))
    r = fc.check_bound(s, e["accepted"], opt, oracle_lib, old, f"emu indefinite {name} reg {e['accepted']}")
    fresh.linear_rollout(1.0, opt)
    rc.fields_equal(s, fresh, len(phases), ["DX"])
    assert all(v <= pc.COND_FACTOR / 2 for k, v in r.items() if k != "share"), r
