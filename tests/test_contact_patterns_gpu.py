"""The whole-body kernels on all 16 contact patterns on the device (cases: tests/pattern_common.py), against the oracle by value.

(a) Per iterate (parity_common.run_steps at its plain tolerances, no arbiter: tests/test_contact_patterns_host.py::test_inputs_qualify shows the
    oracle within 0.05 x the tolerance of its long-double build on every case): three families x 16 patterns, under the default programs and with
    HSDDP_QUAD=0 HSDDP_QUAD_TERMINAL=0 - the lane-quad and one-wave running knots, both terminal programs, the two-wave LQ knot, the sweep and the
    linear rollout on 0 - 4 contact feet and 0 - 4 landing feet.  One larger case, rotate(1101) with 17 problems: a full wave plus a lone quad.
(b) One handle reconfigured through rotate(p) for a sequence of p that shrinks and grows the contact set, two iterates after each: every field
    bit-identical to a fresh handle on that schedule.  The structural zeros of the contact-solve cache are never stored; they rely on the zero
    fill at create and reconfigure, and the window arenas are reused from the third reconfigure on.
(c) Short full solves (2 AL x 3 DDP) of the 16 rotate(p) cases against the oracle with parity_common.compare_solve at its plain tolerances: the
    line-search probe launches, the AL update of the touchdown constraint and the ReB update of the friction pyramid on the odd patterns.  Equal
    counts are a criterion only where the references agree, so the oracle and its long-double build must count alike first.
(d) The simulation walk (k_sim_quad shares the lane-quad contact solve) over the 7 steps of rotate(p), p = 0111, 0001, 1010, on the policies of (c)
    against sim_common.oracle_reference (premise checked in tests/test_contact_patterns_host.py::test_sim_program_walks_odd_patterns)."""
import numpy as np
import pytest

from conftest import pkg
import parity_common as pc
import pattern_common as pt
import sim_common as sc

pytestmark = pytest.mark.gpu

PROGRAMS = {"default": {"HSDDP_QUAD": None, "HSDDP_QUAD_TERMINAL": None}, "one_wave": {"HSDDP_QUAD": "0", "HSDDP_QUAD_TERMINAL": "0"}}
PATTERN_IDS = [pt.name(p) for p in pt.P16]


def _programs(monkeypatch, which):
    """The handle reads these when it is created."""
    for k, v in PROGRAMS[which].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("program", sorted(PROGRAMS))
@pytest.mark.parametrize("p", pt.P16, ids=PATTERN_IDS)
@pytest.mark.parametrize("family", pt.FAMILIES)
def test_pattern_iterates_against_the_oracle(hip_lib, oracle_lib, monkeypatch, family, p, program):
    _programs(monkeypatch, program)
    phases = pt.case(family, p)
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, pt.states())
    try:
        report = pc.run_steps(pkg, so, sg, phases, pkg.mhpc_ddp_setting(), n_iter=2)
        print(f"[patterns] device {program} {family} {pt.name(p)}: error / tolerance {pt.worst_ratio(report)}")
    finally:
        so.close(); sg.close()


def test_pattern_iterates_full_wave_and_lone_quad(hip_lib, oracle_lib, monkeypatch):
    """17 problems: the terminal units of a phase fill a wave and leave a lone quad, as in test_quad_terminal_iterates_against_the_oracle; the
    119 running knots fill seven lane-quad waves and part of an eighth."""
    _programs(monkeypatch, "default")
    phases = pt.case("rotate", (1, 1, 0, 1))
    so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, pt.states(17))
    try:
        report = pc.run_steps(pkg, so, sg, phases, pkg.mhpc_ddp_setting(), n_iter=2)
        print(f"[patterns] device default rotate 1101 batch 17: error / tolerance {pt.worst_ratio(report)}")
    finally:
        so.close(); sg.close()


# ------------------------------------------------------------------------------------------------------------------- (b)
def _stages(opt):
    """The steps of parity_common.run_steps (two iterates) on one handle: (name, call, fields written)."""
    for it in range(2):
        eps = 0.0 if it == 0 else 1.0

        def rollout(s, eps=eps, first=(it == 0)):
            s.hybrid_rollout(eps, opt); s.compute_cost(opt)
            if first:
                s.update_nominal_trajectory()

        def sweep(s):
            assert s.backward_sweep(0.0).all()
        yield f"rollout{it}", rollout, pc.STEP_FIELDS["rollout"]
        yield f"lq{it}", (lambda s: s.LQ_approximation(opt)), pc.STEP_FIELDS["lq"]
        yield f"sweep{it}", sweep, pc.STEP_FIELDS["sweep"]
        yield f"linear{it}", (lambda s: s.linear_rollout(1.0, opt)), pc.STEP_FIELDS["linear"]


def _two_iterates(s, opt, twin=None):
    """Runs the stages on s (and on twin in step); with a twin, every field a stage wrote must be bit-identical on both."""
    for stage, call, fields in _stages(opt):
        call(s)
        if twin is None:
            continue
        call(twin)
        for i in range(len(s.phases)):
            for f in fields:
                a, b = s.field(i, f), twin.field(i, f)
                assert a.shape == b.shape and np.isfinite(a).all(), (stage, i, f)
                assert np.array_equal(a, b), (stage, i, f, float(np.abs(a - b).max()))
        assert np.array_equal(s.info_arrays()["actual_cost"], twin.info_arrays()["actual_cost"]), stage


def _fresh(phases, x0):
    s = pkg.MultiPhaseDDP(phases, batch=x0.shape[0])
    s.set_initial_condition(x0)
    return s


@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_reconfigure_leaves_nothing_of_the_previous_pattern(hip_lib, monkeypatch, program):
    """Every phase of the new window is new to the handle (src_phase = -1: zero trajectory, initial constraint parameters), then given its
    nominal trajectory like a fresh handle's.  The handle's solver counters go on counting across a reconfigure (include/hsddp.h) where a fresh
    handle starts at zero; the step calls used here read none of them, and only fields and the cost are compared."""
    _programs(monkeypatch, program)
    opt = pkg.mhpc_ddp_setting()
    x0 = pt.states()
    first = pt.case("rotate", pt.RECONFIGURE_ORDER[0])
    s = _fresh(first, x0)
    _two_iterates(s, opt)                                      # the handle has run before its first reconfigure
    try:
        for p in pt.RECONFIGURE_ORDER:
            phases = pt.case("rotate", p)
            s.reconfigure(phases, [-1] * len(phases), [0] * len(phases))
            for i, ph in enumerate(phases):
                s.set_nominal(i, ph["Xbar"], ph["Ubar"])
            s.set_initial_condition(x0)
            twin = _fresh(phases, x0)
            try:
                _two_iterates(s, opt, twin)
            except AssertionError as e:
                raise AssertionError(f"after reconfigure to rotate({pt.name(p)}): {e}") from e
            finally:
                twin.close()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------- (c), (d)
@pytest.fixture(scope="module")
def solved(oracle_lib, oracle_ld_lib, hip_lib):
    """rotate(p) solved on the oracle and on the device, once per pattern: p -> (phases, oracle handle, device handle, oracle's info arrays).
    The precondition and the comparison of (c) are made here, when the pair is solved, before anything else touches the handles."""
    cache = {}

    def get(p):
        if p not in cache:
            phases = pt.case("rotate", p)
            x0 = pt.states()
            so, sg = pc.make_pair(pkg, oracle_lib, hip_lib, phases, x0)
            sx = pc.make_exact(pkg, oracle_ld_lib, phases, x0)
            try:
                for s in (so, sx, sg):
                    s.solve(pt.solve_options())
                io, ix = so.info_arrays(), sx.info_arrays()
                for k in pc.COUNT_KEYS:
                    assert np.array_equal(io[k], ix[k]), ("the oracle and its long-double build disagree: not a case for equal counts", pt.name(p), k, io[k], ix[k])
                report = pc.compare_solve(so, sg, len(phases), tag=f"solve rotate {pt.name(p)}")
                print(f"[patterns] device solve rotate {pt.name(p)}: error / tolerance {pt.worst_ratio(report)}, n_iters {io['n_iters'].tolist()}, "
                      f"n_ls_iters {io['n_ls_iters'].tolist()}")
            except BaseException:
                so.close(); sg.close()
                raise
            finally:
                sx.close()
            cache[p] = (phases, so, sg, io)
        return cache[p]
    yield get
    for phases, so, sg, io in cache.values():
        so.close(); sg.close()


@pytest.mark.parametrize("p", pt.P16, ids=PATTERN_IDS)
def test_short_solves_against_the_oracle(solved, monkeypatch, p):
    _programs(monkeypatch, "default")
    phases, so, sg, io = solved(p)
    assert (io["status"] == 0).all(), io["status"]


def test_short_solves_backtrack_somewhere(solved, monkeypatch):
    """The probe launches of the line search ran in the set above: in at least one problem a first step length was refused."""
    _programs(monkeypatch, "default")
    assert any((solved(p)[3]["n_ls_iters"] > solved(p)[3]["n_iters"]).any() for p in pt.P16)


@pytest.mark.parametrize("p", pt.SIM_PATTERNS, ids=[pt.name(p) for p in pt.SIM_PATTERNS])
def test_sim_walks_odd_patterns(solved, monkeypatch, p):
    """Three samples per problem around Xbar[0] over all 7 control knots: a three-, one- or two-foot phase behind a lift-off, then the touchdown
    of rot(p) & ~p.  The device and the oracle each simulate their own solved policy, as test_sim_parity_trot_windows does."""
    _programs(monkeypatch, "default")
    phases, so, sg, io = solved(p)
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 3, 0.02, 0.2, seed=pt.SEED)
    smap = sc.step_map(phases, 7)
    res = sg.simulate(xs, 7, keep_traj=True)
    X, U, xbar = sc.oracle_reference(so, pkg.mhpc_ddp_setting(MS=0), xs, smap)
    assert res["X"].shape == (pt.BATCH, 3, 8, 36) and res["U"].shape == (pt.BATCH, 3, 7, 12)
    sc.compare_window(f"device rotate {pt.name(p)}", res, X, U, xbar)
