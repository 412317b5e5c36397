"""Shared by tests/test_kin_patterns_host.py and tests/test_kin_patterns_gpu.py: kinodynamic (HKD) and single-rigid-body (SRB) windows that put
every one of the 16 contact sets, touchdown sets of every size and contact rows that change from knot to knot and from problem to problem in front
of the foot-indexed code of hkd_knot.hpp and srb_knot.hpp (the pyramid rows through P.feet, the barrier-slot rank a2 of hkd_lq_knot, the running
touchdown index of the two HKD terminal knots, the per-leg reset map and Px, the force sum over contact[l], srb_xdot's ref_contact row).

HKD, p one of pattern_common.P16 (the families of pattern_common on problems.hkd_trot_problem):

  hkd_case("into_stance", p)    schedule (p, 1111),         horizons (3, 2),    last_next 1111   touchdown of ~p (0 - 4 feet) behind a phase on p
  hkd_case("out_of_stance", p)  schedule (1111, p),         horizons (3, 2),    last_next p      lift-off of ~p; the last phase runs on p
  hkd_case("rotate", p)         schedule (1111, p, rot(p)), horizons (2, 3, 2), last_next 1111   lift-off and touchdown at one boundary, asymmetric sets
  states: problems.hkd_ensemble_x0(5, 20241222, phases); option: problems.hkd_ddp_setting()

SRB behind whole-body phases (problems.mhpc_problem), states pattern_common.states(), option mhpc_ddp_setting():

  srb_tail(p)       whole body (1111) x 2 knots, then SRB phases on p x 3 and rot(p) x 2
  srb_handoff(p)    whole body (1111) x 2, (p) x 3 - the reset into the SRB state comes out of a phase on p - then an SRB phase on rot(p) x 3
  srb_knotwise(s)   whole body (1111) x 2, SRB phases of 8 and 9 knots whose ref_contact changes at every knot: row k of SRB phase j is
                    P16[perm[(first_j + k) % 16]], perm = np.random.default_rng(s).permutation(16), first_j = the knots of the SRB phases before j.
                    The 17 rows the dynamics read (k < h) hold all 16 contact sets; a row read at knot 0, or at another knot, is another set.
  srb_per_problem() the same window, one row sequence per problem: problem b > 0 starts the permutation at 3 b, problem 0 keeps the constant rows of
                    its schedule (1001, 0110).  B phase lists that differ in nothing but those rows, and their problems.stack_references stack.

contact_sets() is the coverage helper the tests hold these statements with.  Singles puts B batch-1 handles, each on its own phase list, behind the
interface parity_common.run_steps takes: the oracle has no per-problem references."""
import numpy as np

from conftest import pkg
import pattern_common as pt

P = pkg.problems
MODEL_SRB = pkg.MODEL_SRB
HKD_CASES = [(family, p) for family in pt.FAMILIES for p in pt.P16]
HKD_IDS = [f"{family}-{pt.name(p)}" for family, p in HKD_CASES]
KNOTWISE_SEEDS = (1, 2, 3)
KNOTWISE_HORIZONS = (8, 9)
PER_PROBLEM_SEED = 1
EXPORT_PATTERNS = pt.SIM_PATTERNS                                   # 0111, 0001, 1010
F32_PATTERNS = pt.SIM_PATTERNS + ((0, 0, 0, 0),)
_FAMILY = {"into_stance": pt.into_stance, "out_of_stance": pt.out_of_stance, "rotate": pt.rotate}


def hkd_case(family, p):
    """Phase descriptors of one HKD case."""
    return P.hkd_trot_problem(**_FAMILY[family](p))


def hkd_states(phases, batch=pt.BATCH):
    return P.hkd_ensemble_x0(batch, pt.SEED, phases)


def hkd_solve_options():
    """The short full solves: 2 AL x 3 DDP iterations."""
    return P.hkd_ddp_setting(max_AL_iter=2, max_DDP_iter=3)


def srb_tail(p):
    return P.mhpc_problem(wb_schedule=(pt.STANCE,), wb_horizons=(2,), srb_schedule=(tuple(p), pt.rot(p)), srb_horizons=(3, 2))


def srb_handoff(p):
    return P.mhpc_problem(wb_schedule=(pt.STANCE, tuple(p)), wb_horizons=(2, 3), srb_schedule=(pt.rot(p),), srb_horizons=(3,))


def _knotwise_window():
    return P.mhpc_problem(wb_schedule=(pt.STANCE,), wb_horizons=(2,), srb_horizons=KNOTWISE_HORIZONS)


def _set_rows(phases, perm, start):
    """ref_contact of the SRB phases, in place (the descriptors point at these buffers): one running index over the SRB knots, from `start`."""
    first = start
    for ph in phases:
        if ph["desc"].model != MODEL_SRB:
            continue
        rc = ph["bufs"]["ref_contact"]
        for k in range(rc.shape[0]):
            rc[k] = pt.P16[perm[(first + k) % 16]]
        first += ph["desc"].horizon
    return phases


def srb_knotwise(seed):
    return _set_rows(_knotwise_window(), np.random.default_rng(seed).permutation(16), 0)


def srb_per_problem(batch=pt.BATCH, seed=PER_PROBLEM_SEED):
    """(phase lists [batch], their stack for Solver.set_references)."""
    perm = np.random.default_rng(seed).permutation(16)
    lists = [_knotwise_window() if b == 0 else _set_rows(_knotwise_window(), perm, 3 * b) for b in range(batch)]
    return lists, P.stack_references(lists)


def srb_phases(phases):
    return [i for i, ph in enumerate(phases) if ph["desc"].model == MODEL_SRB]


def contact_sets(phase_lists):
    """{(phase, problem): the contact sets its running knots meet, in knot order} of B phase lists (one list: problem 0).  An SRB knot k < h takes
    its set from row k of ref_contact (the terminal knot has no dynamics), every other phase from its descriptor."""
    if isinstance(phase_lists[0], dict):
        phase_lists = [phase_lists]
    out = {}
    for b, phases in enumerate(phase_lists):
        for i, ph in enumerate(phases):
            d = ph["desc"]
            if d.model == MODEL_SRB:
                out[(i, b)] = tuple(tuple(int(c) for c in row) for row in ph["bufs"]["ref_contact"][:d.horizon])
            else:
                out[(i, b)] = (tuple(int(c) for c in d.contact),) * d.horizon
    return out


def srb_rows(phases):
    """The row sequence of one problem over its SRB phases."""
    sets = contact_sets([phases])
    return tuple(s for i in srb_phases(phases) for s in sets[(i, 0)])


def make(lib, phases, x0, refs=None, **kw):
    """A handle on `phases` with their nominal trajectories; refs: a stack_references stack, set on every phase."""
    s = pkg.Solver(lib, phases, batch=x0.shape[0], **kw)
    for i, ph in enumerate(phases):
        s.set_nominal(i, ph["Xbar"], ph["Ubar"])
    if refs is not None:
        for i, r in enumerate(refs):
            s.set_references(i, **r)
    s.set_initial_condition(x0)
    return s


def two_iterates(s, opt):
    """The steps of parity_common.run_steps (two iterates) on one handle, nothing compared."""
    for it in range(2):
        s.hybrid_rollout(0.0 if it == 0 else 1.0, opt); s.compute_cost(opt)
        if it == 0:
            s.update_nominal_trajectory()
        s.LQ_approximation(opt)
        assert s.backward_sweep(0.0).all()
        s.linear_rollout(1.0, opt)


class Singles:
    """B batch-1 handles of one library, problem b on phase list b, behind the interface of a batch-B Solver (as pw_common.StackedOracle)."""

    def __init__(self, lib, phase_lists, x0):
        self.batch = len(phase_lists)
        self.phases = phase_lists[0]
        self.s = [make(lib, pl, np.ascontiguousarray(x0[b:b + 1])) for b, pl in enumerate(phase_lists)]

    def _all(self, name, *a):
        return [getattr(s, name)(*a) for s in self.s]

    def hybrid_rollout(self, eps, opt): self._all("hybrid_rollout", eps, opt)
    def compute_cost(self, opt): self._all("compute_cost", opt)
    def LQ_approximation(self, opt): self._all("LQ_approximation", opt)
    def linear_rollout(self, eps, opt): self._all("linear_rollout", eps, opt)
    def update_nominal_trajectory(self): self._all("update_nominal_trajectory")
    def backward_sweep(self, reg): return np.concatenate(self._all("backward_sweep", reg))
    def measure_dynamics_feasibility(self): return np.concatenate(self._all("measure_dynamics_feasibility"))

    def get_exp_cost_change(self):
        r = self._all("get_exp_cost_change")
        return np.concatenate([x[0] for x in r]), np.concatenate([x[1] for x in r])

    def info_arrays(self):
        r = self._all("info_arrays")
        return {k: np.concatenate([x[k] for x in r]) for k in r[0]}

    def field(self, phase, name, b0=0, nb=None):
        a = np.concatenate(self._all("field", phase, name), axis=0)
        return a[b0:] if nb is None else a[b0:b0 + nb]

    def close(self):
        self._all("close")
