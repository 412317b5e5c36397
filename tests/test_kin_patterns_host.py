"""CPU tests: the kinodynamic and single-rigid-body kernel programs on every contact set (cases: tests/kin_pattern_common.py), compiled for the host
by the lane emulator tests/_emu, against the oracle - per iterate, at the plain tolerances of parity_common (1e-8 x scale per field, K 1e-6
absolute, scalars 1e-10), without the conditioning arbiter.

* test_coverage: what the case builders promise - every contact set in each knot-wise window, rows of 0 - 4 feet, one row sequence per problem.
* test_inputs_qualify: on every case the fp64 oracle sits within 0.05 x those tolerances of its long-double build, on every field of both
  iterates - so conditioning can neither hide a kernel error nor excuse one, and nothing needs arbitration.
* test_kin_programs_match_oracle: the emulator against the oracle.  The windows with whole-body phases run under both whole-body programs.
* test_per_problem_contact_rows_qualify: the per-problem row sequences, problem by problem (the oracle has no per-problem references).  The
  emulator has no hsddp_set_references either, so the batched handle is held to these references on the device only.
* test_short_solves_count_alike: the precondition of the device's short solves - the oracle and its long-double build take the same decisions.

Real HIP execution of the same cases: tests/test_kin_patterns_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import kin_pattern_common as kp
import parity_common as pc
import pattern_common as pt

QUALIFY = 0.05      # oracle-vs-long-double distance allowed, as a fraction of the plain tolerance
PATTERN_IDS = [pt.name(p) for p in pt.P16]
SRB_CASES = [("tail", p) for p in pt.P16] + [("handoff", p) for p in pt.P16] + [("knotwise", s) for s in kp.KNOTWISE_SEEDS]
SRB_IDS = [f"{kind}-{pt.name(a) if kind != 'knotwise' else a}" for kind, a in SRB_CASES]
CASES = [("hkd-" + family, p) for family, p in kp.HKD_CASES] + SRB_CASES
CASE_IDS = ["hkd-" + i for i in kp.HKD_IDS] + SRB_IDS


def build(kind, arg):
    """(phases, initial states, option) of one case."""
    if kind.startswith("hkd-"):
        phases = kp.hkd_case(kind[4:], arg)
        return phases, kp.hkd_states(phases), pkg.problems.hkd_ddp_setting()
    phases = {"tail": kp.srb_tail, "handoff": kp.srb_handoff, "knotwise": kp.srb_knotwise}[kind](arg)
    return phases, pt.states(), pkg.mhpc_ddp_setting()


def tag_of(kind, arg):
    return f"{kind} {arg if kind == 'knotwise' else pt.name(arg)}"


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "_emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    return pkg._abi.bind(ctypes.CDLL(os.path.join(d, "libhsddp_emu.so")))


def test_coverage():
    every = set(pt.P16)
    for seed in kp.KNOTWISE_SEEDS:
        phases = kp.srb_knotwise(seed)
        rows = kp.srb_rows(phases)
        assert len(rows) == sum(kp.KNOTWISE_HORIZONS) and len(set(rows)) >= 12, (seed, len(set(rows)))
        assert {sum(r) for r in rows} == {0, 1, 2, 3, 4}, seed
        assert all(a != b for a, b in zip(rows, rows[1:])), seed                       # the set changes at every knot
        print(f"[kin patterns] knot-wise seed {seed}: {len(set(rows))} distinct contact sets over {len(rows)} single-rigid-body knots")
    lists, stack = kp.srb_per_problem()
    seqs = [kp.srb_rows(pl) for pl in lists]
    assert len(set(seqs)) == len(lists) == pt.BATCH
    assert set(seqs[0]) == {(1, 0, 0, 1), (0, 1, 1, 0)}                                 # problem 0: the constant rows of its schedule
    for b in range(1, pt.BATCH):
        assert {sum(r) for r in seqs[b]} == {0, 1, 2, 3, 4}, b
    sets = kp.contact_sets(lists)
    for i in kp.srb_phases(lists[0]):
        assert len({sets[(i, b)] for b in range(pt.BATCH)}) == pt.BATCH, i              # per phase, too
        assert np.array_equal(stack[i]["ref_contact"][:, :lists[0][i]["desc"].horizon], np.array([sets[(i, b)] for b in range(pt.BATCH)]))
    met = {c for family, p in kp.HKD_CASES for seq in kp.contact_sets(kp.hkd_case(family, p)).values() for c in seq}
    assert met == every
    td = {sum(1 for a, b in zip(ph["desc"].contact, ph["desc"].next_contact) if not a and b) for family, p in kp.HKD_CASES for ph in kp.hkd_case(family, p)}
    assert td == {0, 1, 2, 3, 4}                                                         # touchdown sets of every size


@pytest.mark.parametrize("kind,arg", CASES, ids=CASE_IDS)
def test_inputs_qualify(oracle_lib, oracle_ld_lib, kind, arg):
    phases, x0, opt = build(kind, arg)
    so, sx = pc.make_pair(pkg, oracle_lib, oracle_ld_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, sx, phases, opt, n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
        print(f"[kin patterns] qualify {tag_of(kind, arg)}: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    finally:
        so.close(); sx.close()


# kinodynamic windows hold no whole-body phase: one run; the others once per whole-body program (HSDDP_EMU_QUAD)
EMU_RUNS = [(k, a, "hkd") for k, a in CASES if k.startswith("hkd-")] + [(k, a, prog) for prog in ("wave", "quad") for k, a in SRB_CASES]
EMU_IDS = [i for i in CASE_IDS if i.startswith("hkd-")] + [f"{i}-{prog}" for prog in ("wave", "quad") for i in SRB_IDS]


@pytest.mark.parametrize("kind,arg,program", EMU_RUNS, ids=EMU_IDS)
def test_kin_programs_match_oracle(emu_lib, oracle_lib, kind, arg, program, monkeypatch):
    if program == "quad":
        monkeypatch.setenv("HSDDP_EMU_QUAD", "1")
    else:
        monkeypatch.delenv("HSDDP_EMU_QUAD", raising=False)
    phases, x0, opt = build(kind, arg)
    so, se = pc.make_pair(pkg, oracle_lib, emu_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, se, phases, opt, n_iter=2)
        print(f"[kin patterns] emulator {program} {tag_of(kind, arg)}: error / tolerance {pt.worst_ratio(report)}")
    finally:
        so.close(); se.close()


def test_knotwise_rows_are_live(oracle_lib):
    """The rows matter: the second iterate's SRB states leave those of the constant-row window by far more than any tolerance."""
    opt = pkg.mhpc_ddp_setting()
    plain = kp.srb_per_problem()[0][0]
    for seed in kp.KNOTWISE_SEEDS:
        phases = kp.srb_knotwise(seed)
        sa, sb = kp.make(oracle_lib, phases, pt.states()), kp.make(oracle_lib, plain, pt.states())
        kp.two_iterates(sa, opt); kp.two_iterates(sb, opt)
        d = max(float(np.abs(sa.field(i, "X") - sb.field(i, "X")).max()) for i in kp.srb_phases(phases))
        print(f"[kin patterns] knot-wise seed {seed}: single-rigid-body states differ from the constant-row window by {d:.3g}")
        assert d > 1e-2, (seed, d)
        sa.close(); sb.close()


@pytest.mark.parametrize("b", range(pt.BATCH))
def test_per_problem_contact_rows_qualify(oracle_lib, oracle_ld_lib, emu_lib, b, monkeypatch):
    """Problem b alone on its own phase list: the reference the device's batched handle is held to qualifies, and the emulator (which has no
    per-problem references: one batch-1 handle per list) meets it at the plain tolerances."""
    monkeypatch.delenv("HSDDP_EMU_QUAD", raising=False)
    lists, _ = kp.srb_per_problem()
    x0 = np.ascontiguousarray(pt.states()[b:b + 1])
    so, sx = pc.make_pair(pkg, oracle_lib, oracle_ld_lib, lists[b], x0)
    try:
        report = pc.run_steps(pkg, so, sx, lists[b], pkg.mhpc_ddp_setting(), n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
        print(f"[kin patterns] qualify per-problem rows, problem {b}: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    finally:
        so.close(); sx.close()
    so, se = pc.make_pair(pkg, oracle_lib, emu_lib, lists[b], x0)
    try:
        report = pc.run_steps(pkg, so, se, lists[b], pkg.mhpc_ddp_setting(), n_iter=2)
        print(f"[kin patterns] emulator per-problem rows, problem {b}: error / tolerance {pt.worst_ratio(report)}")
    finally:
        so.close(); se.close()


@pytest.mark.parametrize("p", pt.P16, ids=PATTERN_IDS)
def test_short_solves_count_alike(oracle_lib, oracle_ld_lib, p):
    """2 AL x 3 DDP iterations of rotate(p): the fp64 oracle and its long-double build agree on every count and end with status 0, so equal counts
    are a fair demand on the device (tests/test_kin_patterns_gpu.py leaves no pattern out)."""
    phases = kp.hkd_case("rotate", p)
    so, sx = pc.make_pair(pkg, oracle_lib, oracle_ld_lib, phases, kp.hkd_states(phases))
    try:
        so.solve(kp.hkd_solve_options()); sx.solve(kp.hkd_solve_options())
        io, ix = so.info_arrays(), sx.info_arrays()
        print(f"[kin patterns] short solve rotate {pt.name(p)}: n_iters {io['n_iters'].tolist()} n_ls_iters {io['n_ls_iters'].tolist()} "
              f"n_reg_iters {io['n_reg_iters'].tolist()} max_tconstr {float(io['max_tconstr'].max()):.3g}")
        for k in pc.COUNT_KEYS:
            assert np.array_equal(io[k], ix[k]), (k, io[k], ix[k])
        assert (io["status"] == 0).all(), io["status"]
        report = pc.compare_solve(so, sx, len(phases), rtol=QUALIFY * 1e-6, atol_K=QUALIFY * 1e-6, tag=f"solve rotate {pt.name(p)}")
        print(f"[kin patterns] short solve rotate {pt.name(p)}: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    finally:
        so.close(); sx.close()
