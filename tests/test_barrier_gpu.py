"""The relaxed barrier on both of its branches, and the parameter updates between augmented-Lagrangian iterations, on the device against the oracle
by value (cases: tests/barrier_common.py; their qualification and coverage: tests/test_barrier_host.py).

(a) Step cases, two iterates of parity_common.run_steps at its plain tolerances, no arbiter - under the default programs and with HSDDP_QUAD=0
    HSDDP_QUAD_TERMINAL=0: reb_barrier / reb_barrier1, q_barrier with its wave-wide shortcut and rcp(delta), wb_constraint_sel, the per-leg
    constraint rows of the lane quad and the barrier derivatives of the three LQ knots with entries above delta, inside and violated.  wb_edges once
    more with 17 problems: a full wave plus a lone quad.
(b) Update cases: solves with update_ReB = 7, update_relax = 0.5 and max_AL_iter = 1 .. 4 (so every intermediate parameter state is compared) -
    compare_solve at its plain 1e-6, and REB_EPS, REB_DELTA and AL_SIGMA equal to the fp64 oracle's bit for bit on every phase (each update is one
    IEEE multiply and one fmax / fmin), AL_LAMBDA at 1e-8 x scale.
(c) The carry across a window shift: after the max_AL_iter = 2 solve of wb_updates both handles are reconfigured to the window one knot later;
    the four fields agree as in (b) and are what barrier_common.expected_after_shift states; one more solve on both, compared as in (b).
(d) fp32 handles on hkd_updates and srb_updates: the parameter fields are plain fp64 arrays and meet the same equality; the solve itself stays with
    the limits of the existing fp32 tests."""
import numpy as np
import pytest

from conftest import pkg
import barrier_common as bc
import parity_common as pc

pytestmark = pytest.mark.gpu

PROGRAMS = {"default": {"HSDDP_QUAD": None, "HSDDP_QUAD_TERMINAL": None}, "one_wave": {"HSDDP_QUAD": "0", "HSDDP_QUAD_TERMINAL": "0"}}


def _programs(monkeypatch, which):
    """The handle reads these when it is created."""
    for k, v in PROGRAMS[which].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("program", sorted(PROGRAMS))
@pytest.mark.parametrize("name", bc.STEP_CASES)
def test_step_cases_against_the_oracle(hip_lib, oracle_lib, monkeypatch, name, program):
    _programs(monkeypatch, program)
    phases, x0 = bc.step_case(name)
    so, sg = bc.make(oracle_lib, phases, x0), bc.make(hip_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, sg, phases, bc.step_option(name), n_iter=2)
        print(f"[barrier] device {program} {name}: error / tolerance {bc.worst_ratio(report)}")
    finally:
        so.close(); sg.close()


def test_wb_edges_full_wave_and_lone_quad(hip_lib, oracle_lib, monkeypatch):
    """17 problems x 7 running knots: seven lane-quad waves and part of an eighth; the terminal units of a phase fill a wave and leave a lone quad.
    Problems 6 and 13 are plain ensemble states."""
    _programs(monkeypatch, "default")
    phases, x0 = bc.step_case("wb_edges", batch=17)
    so, sg = bc.make(oracle_lib, phases, x0), bc.make(hip_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, sg, phases, bc.step_option("wb_edges"), n_iter=2)
        print(f"[barrier] device default wb_edges batch 17: error / tolerance {bc.worst_ratio(report)}")
    finally:
        so.close(); sg.close()


# ------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("n_al", bc.AL_ITERS)
@pytest.mark.parametrize("name", bc.UPDATE_CASES)
def test_update_solves_against_the_oracle(hip_lib, oracle_lib, monkeypatch, name, n_al):
    _programs(monkeypatch, "default")
    phases, x0, option = bc.update_case(name)
    so, sg = bc.make(oracle_lib, phases, x0), bc.make(hip_lib, phases, x0)
    try:
        so.solve(option(n_al)); sg.solve(option(n_al))
        report = pc.compare_solve(so, sg, len(phases), tag=f"{name} max_AL_iter {n_al}")
        print(f"[barrier] device solve {name} max_AL_iter {n_al}: error / tolerance {bc.worst_ratio(report)}")
        bc.compare_params(so, sg, f"{name} max_AL_iter {n_al}")
    finally:
        so.close(); sg.close()


# ------------------------------------------------------------------------------------------------------------------- (c)
def test_parameters_carry_across_a_window_shift(hip_lib, oracle_lib, monkeypatch):
    _programs(monkeypatch, "default")
    phases, x0, option = bc.update_case("wb_updates")
    so, sg = bc.make(oracle_lib, phases, x0), bc.make(hip_lib, phases, x0)
    try:
        so.solve(option(2)); sg.solve(option(2))
        bc.compare_params(so, sg, "before the shift")
        before = bc.params(sg)
        new = bc.shift_window(so); bc.shift_window(sg)
        bc.compare_params(so, sg, "after the shift")
        want, got = bc.expected_after_shift(before, new, x0.shape[0]), bc.params(sg)
        for f in bc.PARAM_FIELDS:
            for i in range(len(new)):
                assert np.array_equal(got[f][i], want[f][i]), (f, i)
        so.solve(option(2)); sg.solve(option(2))
        report = pc.compare_solve(so, sg, len(new), tag="wb_updates after the window shift")
        print(f"[barrier] device solve wb_updates after the window shift: error / tolerance {bc.worst_ratio(report)}")
        bc.compare_params(so, sg, "second solve")
    finally:
        so.close(); sg.close()


# ------------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("n_al", bc.AL_ITERS)
@pytest.mark.parametrize("name", ("hkd_updates", "srb_updates"))
def test_fp32_handles_update_parameters_alike(hip_lib, oracle_lib, monkeypatch, name, n_al):
    _programs(monkeypatch, "default")
    phases, x0, option = bc.update_case(name)
    so, sg = bc.make(oracle_lib, phases, x0), bc.make(hip_lib, phases, x0, precision=pkg.PREC_F32)
    try:
        so.solve(option(n_al)); sg.solve(option(n_al))
        io, ig = so.info_arrays(), sg.info_arrays()
        print(f"[barrier] fp32 {name} max_AL_iter {n_al}: counts oracle / fp32 { {k: (io[k].tolist(), ig[k].tolist()) for k in pc.COUNT_KEYS} }")
        bc.compare_params(so, sg, f"fp32 {name} max_AL_iter {n_al}")
    finally:
        so.close(); sg.close()
