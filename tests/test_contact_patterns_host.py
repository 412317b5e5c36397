"""CPU tests: the whole-body kernel programs on all 16 contact patterns (tests/pattern_common.py), compiled for the host by the lane emulator
tests/_emu, against the oracle - per iterate, at the plain tolerances of parity_common (1e-8 x scale per field, K 1e-6 absolute, scalars 1e-10),
without the conditioning arbiter.

* test_inputs_qualify: on every case the fp64 oracle sits within 0.05 x those tolerances of its long-double build, on every field of both
  iterates - so conditioning can neither hide a kernel error nor excuse one, and nothing needs arbitration.
* test_pattern_programs_match_oracle: pattern x family x program (the one-wave knot, the lane quad).
* test_quad_terminal_on_every_touchdown_set: the lane-quad terminal knot (wb_quad_term.hpp through tests/_emu/term_emu.cpp) against the one-wave
  terminal knot on touchdown sets of 0 - 4 feet.
* test_sim_program_walks_odd_patterns: the simulation program (wb_sim.hpp through tests/_emu/sim_emu.cpp) over the 7 steps of rotate(p) for
  p = 0111, 0001, 1010 against the oracle's window (tests/sim_common.py), after checking that file's premise on these windows.

Real HIP execution of the same cases: tests/test_contact_patterns_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import parity_common as pc
import pattern_common as pt
import sim_common as sc
import term_common as tc
from test_sim_host import emu_simulate, to_result      # the driver of tests/_emu/sim_emu.cpp: it takes the schedule from the handle's phases

QUALIFY = 0.05      # oracle-vs-long-double distance allowed, as a fraction of the plain tolerance
CASES = [(family, p) for family in pt.FAMILIES for p in pt.P16]
CASE_IDS = [f"{family}-{pt.name(p)}" for family, p in CASES]


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "_emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    return pkg._abi.bind(ctypes.CDLL(os.path.join(d, "libhsddp_emu.so")))


@pytest.fixture(scope="module")
def sim_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pattern_sim_emu") / "libhsddp_sim_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "sim_emu.cpp"), "-o", out])
    return ctypes.CDLL(out)


@pytest.mark.parametrize("family,p", CASES, ids=CASE_IDS)
def test_inputs_qualify(oracle_lib, oracle_ld_lib, family, p):
    phases = pt.case(family, p)
    so, sx = pc.make_pair(pkg, oracle_lib, oracle_ld_lib, phases, pt.states())
    report = pc.run_steps(pkg, so, sx, phases, pkg.mhpc_ddp_setting(), n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
    print(f"[patterns] qualify {family} {pt.name(p)}: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    so.close(); sx.close()


@pytest.mark.parametrize("program", ["wave", "quad"])
@pytest.mark.parametrize("family,p", CASES, ids=CASE_IDS)
def test_pattern_programs_match_oracle(emu_lib, oracle_lib, family, p, program, monkeypatch):
    if program == "quad":
        monkeypatch.setenv("HSDDP_EMU_QUAD", "1")
    else:
        monkeypatch.delenv("HSDDP_EMU_QUAD", raising=False)
    phases = pt.case(family, p)
    so, se = pc.make_pair(pkg, oracle_lib, emu_lib, phases, pt.states())
    report = pc.run_steps(pkg, so, se, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[patterns] emulator {program} {family} {pt.name(p)}: error / tolerance {pt.worst_ratio(report)}")
    so.close(); se.close()


@pytest.fixture(scope="module")
def term_emu(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("pattern_term_emu"))


@pytest.mark.parametrize("family,p", [c for c in CASES if c[0] != "out_of_stance"], ids=[i for i in CASE_IDS if not i.startswith("out_of_stance")])
def test_quad_terminal_on_every_touchdown_set(term_emu, family, p):
    """The lane-quad terminal knot (wb_quad_term.hpp) is not part of the emulator's rollout; its host form is driven by tests/_emu/term_emu.cpp
    slot by slot against the one-wave terminal knot, which the test above holds to the oracle on the same schedules.  Touchdown sets ~p of 0 - 4
    feet (into_stance) and rot(p) & ~p behind a phase on p (rotate); AL on with per-problem parameters, step lengths 1 and one per problem.
    Compared as tests/test_quad_terminal_host.py does, at its tolerance (1e-11 x max(1, scale): the same arithmetic, sums associated differently):
    the slot partials, X[h], Phibase, Phi, th and the successor's Xsim[0] and Defect[0]."""
    lib, raw = term_emu
    phases = pt.case(family, p)
    x0 = pt.states()
    opt = pkg.mhpc_ddp_setting()
    pair = []
    for _ in range(2):
        s = pkg.Solver(lib, phases, batch=pt.BATCH)
        for i, ph in enumerate(phases):
            s.set_nominal(i, ph["Xbar"], ph["Ubar"])
        s.set_initial_condition(x0)
        s.hybrid_rollout(0.0, opt); s.update_nominal_trajectory(); s.LQ_approximation(opt)
        assert s.backward_sweep(0.0).all()
        s.linear_rollout(1.0, opt)
        for i in range(len(phases)):
            raw.term_emu_set_al(s.h, i, 10.0, 0.75, 0.3, -0.04)
        pair.append(s)
    sw, sq = pair

    def close(tag, a, b):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), tag
        m = ~np.isnan(a)
        if m.any():
            err = np.abs(a[m] - b[m]).max(); scale = max(1.0, np.abs(a[m]).max())
            assert err <= 1e-11 * scale, f"{tag}: |diff| = {err:.3e} > {1e-11 * scale:.3e} (scale {scale:.3e})"
    assert (~np.isnan(tc.terminal(raw, sq, tc.QUAD, np.ones(pt.BATCH), opt, False)[0, :, 0])).all()      # every terminal slot is the quad path's
    for name, eps in (("1", np.ones(pt.BATCH)), ("from_state", 0.5 ** np.arange(pt.BATCH))):
        tag = f"{family} {pt.name(p)} eps={name}"
        ww = tc.terminal(raw, sw, tc.WAVE, eps, opt, True)
        wq = tc.terminal(raw, sq, tc.QUAD, eps, opt, True)
        for q, what in enumerate(("cost", "dsq", "maxh", "ming")):
            close(f"{tag} {what}", ww[..., q], wq[..., q])
        a, b = tc.state(raw, sw), tc.state(raw, sq)
        for i, ph in enumerate(phases):
            d = ph["desc"]; h = d.horizon
            ntd = sum(1 for l in range(4) if d.contact[l] == 0 and d.next_contact[l] == 1)
            close(f"{tag} phase {i} X[h]", a[i]["X"][:, h], b[i]["X"][:, h])
            close(f"{tag} phase {i} records", a[i]["REC"], b[i]["REC"])
            assert (~np.isnan(b[i]["REC"][0, 2:])).sum() == ntd, (tag, i)      # one touchdown constraint per landing foot
            if i > 0:
                close(f"{tag} phase {i} Xsim[0]", a[i]["XSIM"][:, 0], b[i]["XSIM"][:, 0])
                close(f"{tag} phase {i} Defect[0]", a[i]["DEFECT"][:, 0], b[i]["DEFECT"][:, 0])
            if i + 1 < len(phases) and ntd > 0:      # an impact changed the velocities handed to the successor
                assert np.abs(b[i + 1]["XSIM"][:, 0, 18:] - b[i]["X"][:, h, 18:]).max() > 1e-6, (tag, i)
    sw.close(); sq.close()


def _solved(lib, phases, x0):
    s = pkg.Solver(lib, phases, batch=x0.shape[0])
    for i, ph in enumerate(phases):
        s.set_nominal(i, ph["Xbar"], ph["Ubar"])
    s.set_initial_condition(x0); s.solve(pt.solve_options())
    return s


@pytest.mark.parametrize("p", pt.SIM_PATTERNS, ids=[pt.name(p) for p in pt.SIM_PATTERNS])
def test_sim_program_walks_odd_patterns(sim_emu, oracle_lib, oracle_ld_lib, p):
    """The lane-quad contact solve of the simulation walk on three-, one- and two-foot phases with a touchdown of one or two feet under way.
    First the premise of sim_common: the oracle's window within 1e-12 (of the field's scale) of its long-double build's."""
    phases = pt.case("rotate", p)
    so, sx = _solved(oracle_lib, phases, pt.states()), _solved(oracle_ld_lib, phases, pt.states())
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=pt.SEED)
    smap = sc.step_map(phases, 7)
    assert smap[2].sum() == (1 if any(b and not a for a, b in zip(p, pt.rot(p))) else 0)      # the touchdown boundary lies inside the window
    opt_ss = pkg.mhpc_ddp_setting(MS=0)
    X, U, xbar = sc.oracle_reference(so, opt_ss, xs, smap)
    Xx, Ux, _ = sc.oracle_reference(sx, opt_ss, xs, smap)
    for tag, a, b in (("X", X, Xx), ("U", U, Ux)):
        own = float(np.abs(a - b).max()); scale = max(1.0, float(np.abs(a).max()))
        print(f"[patterns] sim premise rotate {pt.name(p)} {tag}: oracle-vs-long-double {own:.3e}, scale {scale:.3e}")
        assert own <= 1e-12 * scale, (tag, own, scale)
    assert np.abs(X[:, :, 1:] - xbar[:, None, 1:]).max() > 1e-3          # the samples do leave the plan
    outs = [emu_simulate(sim_emu, so, b, xs[b], smap) for b in range(pt.BATCH)]
    res = to_result(*[np.stack([o[i] for o in outs]) for i in range(4)])
    sc.compare_window(f"host rotate {pt.name(p)}", res, X, U, xbar)
    so.close(); sx.close()
