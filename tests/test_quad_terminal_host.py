"""CPU test: the lane-quad TERMINAL knot (cafe-mpc_amd/csrc/wb_quad_term.hpp, its host form: the four lanes of a quad as a four-wide value) against
the one-wave terminal knot (wb_knot.hpp: wb_rollout_terminal) under the lane emulator, slot by slot.

Both programs evaluate the same terminal slots of two handles in the same state - one rollout, LQ approximation, backward sweep and linear rollout
in, so that Xbar, dX and the successor's rows are those of a real line search - with per-problem AL parameters (sigma and lambda differ per problem
and touchdown foot, lambda non-zero) at step lengths 1, 0.25 and a different one per problem (the commit launch's `from_state`), writing and probing,
AL on and off.  Compared: the slot partials (cost, squared defect, max |h|, min g = 0), X[h], Phibase, Phi, th, and the successor's Xsim[0] and
Defect[0].  A probe must leave every trajectory and record of the handle untouched, bit for bit.

Tolerance: 1e-11 x max(1, scale of the quantity), the bound test_quad_probe_matches_the_one_wave_knot_slot_by_slot holds the running knot to: the two
programs do the same arithmetic with sums associated differently (pairwise over the quad instead of lane 0's running sum, the block form of the
impulse solve instead of the dense one).

Schedules: a two-foot touchdown (1,0,0,1) -> (0,1,1,0) whose last phase ends in a two-foot touchdown WITHOUT a successor; a four-foot touchdown after
flight (1,1,1,1) -> (0,0,0,0) -> (1,1,1,1), whose first phase ends without a touchdown (lift-off: no impact, v+ = v) and whose last phase has neither
a touchdown nor a successor.  Horizons 1-3; 1, 3 and 17 problems."""
import numpy as np
import pytest

from conftest import pkg
import term_common as tc

RTOL = 1e-11
CASES = {
    "two_foot_touchdown": dict(schedule=((1, 0, 0, 1), (0, 1, 1, 0)), horizons=(2, 3), last_next=(1, 0, 0, 1)),
    "four_foot_touchdown_after_flight": dict(schedule=((1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1)), horizons=(1, 2, 3), last_next=(1, 1, 1, 1)),
}


@pytest.fixture(scope="module")
def term_emu(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("term_emu"))


def _close(tag, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    if a.size == 0:
        return
    assert np.array_equal(np.isnan(a), np.isnan(b)), tag
    m = ~np.isnan(a)
    if not m.any():
        return
    err = np.abs(a[m] - b[m]).max(); sc = max(1.0, np.abs(a[m]).max())
    assert err <= RTOL * sc, f"{tag}: |diff| = {err:.3e} > {RTOL * sc:.3e} (scale {sc:.3e})"


def _prepared(lib, raw, phases, x0, opt):
    s = pkg.Solver(lib, phases, batch=x0.shape[0])
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    s.hybrid_rollout(0.0, opt); s.update_nominal_trajectory(); s.LQ_approximation(opt)
    assert s.backward_sweep(0.0).all()
    s.linear_rollout(1.0, opt)
    for i in range(len(phases)):
        raw.term_emu_set_al(s.h, i, 10.0, 0.75, 0.3, -0.04)
    return s


@pytest.mark.parametrize("batch", [1, 3, 17])
@pytest.mark.parametrize("case", sorted(CASES))
def test_quad_terminal_matches_the_one_wave_terminal_slot_by_slot(term_emu, case, batch):
    lib, raw = term_emu
    phases = pkg.problems.wb_trot_problem(**CASES[case])
    nph = len(phases)
    x0 = pkg.problems.wb_ensemble_x0(batch, 20241222)
    opt0 = pkg.mhpc_ddp_setting()
    sw, sq = (_prepared(lib, raw, phases, x0, opt0) for _ in range(2))
    assert max(np.abs(sq.field(i, "DX")).max() for i in range(nph)) > 1e-3      # the step is not a null step
    own = ~np.isnan(tc.terminal(raw, sq, tc.QUAD, np.ones(batch), opt0, False)[0, :, 0])
    assert own.all()      # every terminal slot of these schedules is the quad path's
    steps = {"1": np.ones(batch), "0.25": np.full(batch, 0.25), "from_state": 0.5 ** np.arange(batch)}      # from_state: every problem its own step
    for al in (1, 0):
        opt = pkg.mhpc_ddp_setting(AL_active=al)
        for name, eps in steps.items():
            tag = f"{case} B={batch} AL={al} eps={name}"
            # probe: partials only, nothing of the handle moves
            before = tc.state(raw, sq)
            pq = tc.terminal(raw, sq, tc.QUAD, eps, opt, False)
            after = tc.state(raw, sq)
            for i in range(nph):
                for k in before[i]:
                    assert np.array_equal(before[i][k], after[i][k], equal_nan=True), (tag, "probe wrote", i, k)
            pw = tc.terminal(raw, sw, tc.WAVE, eps, opt, False)
            for q, what in enumerate(("cost", "dsq", "maxh", "ming")):
                _close(f"{tag} probe {what}", pw[..., q], pq[..., q])
            # trial: the same partials and everything the terminal knot stores
            ww = tc.terminal(raw, sw, tc.WAVE, eps, opt, True)
            wq = tc.terminal(raw, sq, tc.QUAD, eps, opt, True)
            assert np.array_equal(pq, wq), tag      # writing does not change what the quad program returns
            for q, what in enumerate(("cost", "dsq", "maxh", "ming")):
                _close(f"{tag} {what}", ww[..., q], wq[..., q])
            a, b = tc.state(raw, sw), tc.state(raw, sq)
            for i in range(nph):
                h = phases[i]["desc"].horizon
                _close(f"{tag} phase {i} X[h]", a[i]["X"][:, h], b[i]["X"][:, h])
                for q, what in enumerate(("Phibase", "Phi", "th0", "th1", "th2", "th3")):
                    _close(f"{tag} phase {i} {what}", a[i]["REC"][:, q], b[i]["REC"][:, q])
                if i > 0:
                    _close(f"{tag} phase {i} Xsim[0]", a[i]["XSIM"][:, 0], b[i]["XSIM"][:, 0])
                    _close(f"{tag} phase {i} Defect[0]", a[i]["DEFECT"][:, 0], b[i]["DEFECT"][:, 0])
                # and nothing else of the trajectories: the running knots' rows are what the preparation left in both handles
                assert np.array_equal(a[i]["X"][:, :h], b[i]["X"][:, :h]) and np.array_equal(a[i]["XSIM"][:, 1:], b[i]["XSIM"][:, 1:]), (tag, i)
            if al == 1 and name == "1":      # the cases exercise what they claim to
                rec = b
                ntd = [sum(1 for l in range(4) if p["desc"].contact[l] == 0 and p["desc"].next_contact[l] == 1) for p in phases]
                for i in range(nph):
                    assert (~np.isnan(rec[i]["REC"][0, 2:])).sum() == ntd[i], (tag, i)
                    assert (wq[:, i, 2] > 0).all() == (ntd[i] > 0), (tag, i)
                    if ntd[i] > 0:      # the AL terms are in Phi
                        assert (np.abs(rec[i]["REC"][:, 1] - rec[i]["REC"][:, 0]) > 1e-9).all(), (tag, i)
                    if i + 1 < nph and ntd[i] > 0:      # an impact changed the velocities handed to the successor
                        assert np.abs(rec[i + 1]["XSIM"][:, 0, 18:] - rec[i]["X"][:, phases[i]["desc"].horizon, 18:]).max() > 1e-6, (tag, i)
                    if i + 1 < nph and ntd[i] == 0:
                        assert np.array_equal(rec[i + 1]["XSIM"][:, 0], rec[i]["X"][:, phases[i]["desc"].horizon]), (tag, i)
    sw.close(); sq.close()
