"""The kinodynamic (HKD) and single-rigid-body (SRB) kernels on every contact set on the device (cases: tests/kin_pattern_common.py), against the
oracle by value.

(a) Per iterate (parity_common.run_steps at its plain tolerances, no arbiter: tests/test_kin_patterns_host.py::test_inputs_qualify shows the oracle
    within 0.05 x the tolerance of its long-double build on every case): the 48 HKD windows, rotate(1101) once more with 17 problems, and the SRB
    tail, hand-off and knot-wise windows under the default programs and with HSDDP_QUAD=0 HSDDP_QUAD_TERMINAL=0 (they hold whole-body phases).
(b) Per-problem contact rows (include/hsddp_refs.h): one handle whose five problems read five different ref_contact sequences, against five
    single-problem oracle handles, bit-identical to five batch-1 device handles, and far from a handle that shares problem 0's rows.
(c) One HKD handle reconfigured through rotate(p) for a sequence of p that shrinks and grows the contact set, two iterates after each: every field
    bit-identical to a fresh handle on that schedule - the ng, nt and feet tables of a smaller set hold nothing of a larger one.
(d) Short full solves (2 AL x 3 DDP) of the 16 HKD rotate(p) windows against the oracle, parity_common.compare_solve at its defaults: the line
    search, the AL update of the touchdown heights and the ReB update of the force pyramid on the odd sets.  The oracle and its long-double build
    count alike on all 16 (tests/test_kin_patterns_host.py::test_short_solves_count_alike), so none is left out.
(e) fp32 handles on rotate(p), p = 0111, 0001, 1010, 0000, first iterate: the record fields are np.float32 of the fp64 twin's bit for bit.
(f) The HKD command export after the solves of (d) on p = 0111, 0001, 1010: rows word for word hkd_command.pack_rows, contacts and footholds
    decoded and held to the schedule - legs without a later foothold in the window (pf_in) and legs whose next foothold lies two phases on."""
import numpy as np
import pytest

from conftest import pkg
import f32_common as fc
import kin_pattern_common as kp
import parity_common as pc
import pattern_common as pt
from test_contact_patterns_gpu import _two_iterates
from test_hkd_command_gpu import check_bit_equal, hkd_command
from test_refs_gpu import assert_problem_equal

pytestmark = pytest.mark.gpu

PATTERN_IDS = [pt.name(p) for p in pt.P16]
SRB_CASES = [("tail", p) for p in pt.P16] + [("handoff", p) for p in pt.P16] + [("knotwise", s) for s in kp.KNOTWISE_SEEDS]
SRB_IDS = [f"{kind}-{pt.name(a) if kind != 'knotwise' else a}" for kind, a in SRB_CASES]
ALL_FIELDS = [f for fields in pc.STEP_FIELDS.values() for f in fields]


@pytest.fixture(params=["default", "wave"])
def programs(request, monkeypatch):
    """The whole-body rollout programs of the handles a test creates: the environment is read when a handle is made."""
    for k in ("HSDDP_QUAD", "HSDDP_QUAD_TERMINAL"):
        if request.param == "wave":
            monkeypatch.setenv(k, "0")
        else:
            monkeypatch.delenv(k, raising=False)
    return request.param


def _parity(oracle_lib, hip_lib, phases, x0, opt, tag):
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, sg, phases, opt, n_iter=2)
        print(f"[kin patterns] device {tag}: error / tolerance {pt.worst_ratio(report)}")
    finally:
        so.close(); sg.close()


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("family,p", kp.HKD_CASES, ids=kp.HKD_IDS)
def test_hkd_iterates_against_the_oracle(hip_lib, oracle_lib, family, p):
    phases = kp.hkd_case(family, p)
    _parity(oracle_lib, hip_lib, phases, kp.hkd_states(phases), pkg.problems.hkd_ddp_setting(), f"hkd {family} {pt.name(p)}")


def test_hkd_iterates_with_17_problems(hip_lib, oracle_lib):
    phases = kp.hkd_case("rotate", (1, 1, 0, 1))
    _parity(oracle_lib, hip_lib, phases, kp.hkd_states(phases, 17), pkg.problems.hkd_ddp_setting(), "hkd rotate 1101 batch 17")


@pytest.mark.parametrize("kind,arg", SRB_CASES, ids=SRB_IDS)
def test_srb_iterates_against_the_oracle(hip_lib, oracle_lib, programs, kind, arg):
    phases = {"tail": kp.srb_tail, "handoff": kp.srb_handoff, "knotwise": kp.srb_knotwise}[kind](arg)
    _parity(oracle_lib, hip_lib, phases, pt.states(), pkg.mhpc_ddp_setting(), f"{programs} {kind} {arg if kind == 'knotwise' else pt.name(arg)}")


# ------------------------------------------------------------------------------------------------------------------- (b)
def test_per_problem_contact_rows(hip_lib, oracle_lib, programs):
    lists, stack = kp.srb_per_problem()
    x0, opt = pt.states(), pkg.mhpc_ddp_setting()
    srb = kp.srb_phases(lists[0])
    so = kp.Singles(oracle_lib, lists, x0)
    sg = kp.make(hip_lib, lists[0], x0, refs=stack)
    ones = kp.Singles(hip_lib, lists, x0)
    shared = kp.make(hip_lib, lists[0], x0)
    try:
        for i in srb:
            assert np.array_equal(sg.get_references(i)["ref_contact"], stack[i]["ref_contact"])
        report = pc.run_steps(pkg, so, sg, lists[0], opt, n_iter=2)
        print(f"[kin patterns] device {programs} per-problem rows: error / tolerance {pt.worst_ratio(report)}")
        kp.two_iterates(ones, opt)
        for b, one in enumerate(ones.s):
            assert_problem_equal(sg, b, one, 0, f"problem {b}")
            for i in range(len(lists[0])):
                for f in ALL_FIELDS:
                    x, y = sg.field(i, f, b, 1), one.field(i, f)
                    assert np.array_equal(x, y), (b, i, f, float(np.abs(x - y).max()) if x.size else 0.0)
        kp.two_iterates(shared, opt)                                        # the guard: a handle on which every problem reads problem 0's rows
        assert_problem_equal(sg, 0, shared, 0, "problem 0 keeps the constant rows")
        for b in range(1, pt.BATCH):
            ratio = max(float(np.abs(sg.field(i, "X", b, 1) - shared.field(i, "X", b, 1)).max()) / (1e-8 * max(1.0, float(np.abs(sg.field(i, "X")).max()))) for i in srb)
            print(f"[kin patterns] device {programs} per-problem rows: problem {b} leaves the shared-row handle by {ratio:.3g} x its tolerance")
            assert ratio > 100.0, (b, ratio)
    finally:
        for s in (so, sg, ones, shared):
            s.close()


# ------------------------------------------------------------------------------------------------------------------- (c)
def test_reconfigure_leaves_nothing_of_the_previous_contact_set(hip_lib):
    """Every phase of the new window is new to the handle (src_phase = -1), then given its nominal trajectory like a fresh handle's; only fields and
    the cost are compared (the solver counters go on counting across a reconfigure)."""
    opt = pkg.problems.hkd_ddp_setting()
    first = kp.hkd_case("rotate", pt.RECONFIGURE_ORDER[0])
    x0 = kp.hkd_states(first)
    s = pkg.MultiPhaseDDP(first, batch=pt.BATCH)
    s.set_initial_condition(x0)
    _two_iterates(s, opt)                                      # the handle has run before its first reconfigure
    try:
        for p in pt.RECONFIGURE_ORDER:
            phases = kp.hkd_case("rotate", p)
            s.reconfigure(phases, [-1] * len(phases), [0] * len(phases))
            for i, ph in enumerate(phases):
                s.set_nominal(i, ph["Xbar"], ph["Ubar"])
            s.set_initial_condition(x0)
            twin = pkg.MultiPhaseDDP(phases, batch=pt.BATCH)
            twin.set_initial_condition(x0)
            try:
                _two_iterates(s, opt, twin)
            except AssertionError as e:
                raise AssertionError(f"after reconfigure to rotate({pt.name(p)}): {e}") from e
            finally:
                twin.close()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------- (d), (f)
@pytest.fixture(scope="module")
def solved(oracle_lib, hip_lib):
    """rotate(p) solved on the oracle and on the device, once per pattern: p -> (phases, device handle, oracle's info arrays).  The comparison of
    (d) is made here, when the pair is solved, before anything else touches the handles."""
    cache = {}

    def get(p):
        if p not in cache:
            phases = kp.hkd_case("rotate", p)
            so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, kp.hkd_states(phases))
            try:
                so.solve(kp.hkd_solve_options()); sg.solve(kp.hkd_solve_options())
                io = so.info_arrays()
                report = pc.compare_solve(so, sg, len(phases), tag=f"solve rotate {pt.name(p)}")
                print(f"[kin patterns] device solve rotate {pt.name(p)}: error / tolerance {pt.worst_ratio(report)}, n_iters {io['n_iters'].tolist()}, "
                      f"n_ls_iters {io['n_ls_iters'].tolist()}")
            except BaseException:
                sg.close()
                raise
            finally:
                so.close()
            cache[p] = (phases, sg, io)
        return cache[p]
    yield get
    for phases, sg, io in cache.values():
        sg.close()


@pytest.mark.parametrize("p", pt.P16, ids=PATTERN_IDS)
def test_short_solves_against_the_oracle(solved, p):
    phases, sg, io = solved(p)
    assert (io["status"] == 0).all(), io["status"]
    assert np.array_equal(sg.info_arrays()["status"], io["status"])


@pytest.mark.parametrize("p", kp.EXPORT_PATTERNS, ids=[pt.name(p) for p in kp.EXPORT_PATTERNS])
def test_command_export_on_asymmetric_schedules(solved, p):
    """All 7 control knots of the window, so the message walks through the three phases."""
    phases, sg, io = solved(p)
    st = np.arange(len(phases) * 4, dtype=np.float64).reshape(-1, 4) * 0.05 + 0.1
    rows, pf, kw = check_bit_equal(sg, st, pt.BATCH, 7, 20241222)
    d = hkd_command.decode(rows)
    schedule = [pt.STANCE, tuple(p), pt.rot(p)]
    walk = hkd_command.step_map([2, 3, 2], 7)
    assert [i for i, _ in walk] == [0, 0, 1, 1, 1, 2, 2]
    for k, (i, _) in enumerate(walk):
        assert np.array_equal(d["contacts"][:, k], np.tile(np.array(schedule[i], dtype=np.int32), (pt.BATCH, 1))), k
    fh = hkd_command.foothold_phases(schedule)
    assert fh == [2 if (not p[l] and pt.rot(p)[l]) else -1 for l in range(4)]      # a landing two phases on, or no foothold in the window
    assert -1 in fh and 2 in fh
    for l in range(4):
        want = pf[:, 3 * l:3 * l + 3] if fh[l] < 0 else sg.field(fh[l], "XBAR")[:, 0, 12 + 3 * l:15 + 3 * l].astype(np.float32)
        assert np.array_equal(d["foot_placement"][:, 3 * l:3 * l + 3], want), l
    assert len({d["foot_placement"][b].tobytes() for b in range(pt.BATCH)}) == pt.BATCH      # one row per problem, not one row five times


# ------------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("p", kp.F32_PATTERNS, ids=[pt.name(p) for p in kp.F32_PATTERNS])
def test_f32_records_are_the_rounded_twin(hip_lib, p):
    phases = kp.hkd_case("rotate", p)
    x0, opt = kp.hkd_states(phases), pkg.problems.hkd_ddp_setting()
    s32, s64 = fc.make(hip_lib, phases, x0, precision=fc.F32), fc.make(hip_lib, phases, x0)
    try:
        fc.prepare(s32, opt); fc.prepare(s64, opt)
        fc.check_records(s32, s64, f"hip rotate {pt.name(p)}")
    finally:
        s32.close(); s64.close()
