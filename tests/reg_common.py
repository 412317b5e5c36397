"""Shared pieces of the regularised-sweep tests (test_reg_sweep_host.py, test_reg_sweep_gpu.py).

The regularisation `reg` enters the Riccati sweep on the diagonals of Qxx and Quu (SinglePhase.cpp:364-365, "quirk x" for Qxx) and
MultiPhaseDDP::backward_sweep_regularized (MultiPhaseDDP.cpp:136-165) repeats the sweep on a LADDER of values until a factorisation passes.
Here: the ladder, the critical reg of a problem (bisection), problems whose Quu is indefinite at reg = 0 with a known critical value, and
the comparison of two backends after a sweep at a given reg.

Indefinite inputs: a negative control weight desc.r[i] = r < 0 puts r dt on the diagonal of luu, so the smallest reg at which every knot
factorises is -r dt (the B^T H B part is of order dt^2 and positive).  A value test must not sit near the accept / reject boundary of a rung,
where a rounding error decides which rung is taken: check_margins() demands that the rung below the critical value is <= 0.8 x and the rung
above >= 1.25 x the critical value, for the first and for the second DDP iteration of a solve (whose ladder starts at accepted / 20).  With
rungs 1e-3 2^k and the second ladder 1e-3 2^k / 20 x 2^j both conditions hold only for a critical value in [1.25, 1.28] x a rung once the
second ladder stays above its 1e-3 floor: the whole-body cases therefore use r = -32.4 (critical 0.324; rejected 0.256 = 0.79 x, accepted
0.512 = 1.58 x; second iteration 0.0256 .. 0.2048 = 0.63 x rejected, 0.4096 = 1.264 x accepted).  r = -30 (critical 0.3) would leave the
rejected rung 0.256 at 0.853 x the critical value, outside the margin.  The small critical values (0.003, 0.0031) fall back on the floor in the
second iteration (0.0002, 0.001, 0.002, 0.004) and keep the margins of the first.
"""
import numpy as np

from conftest import pkg
import parity_common as pc

REGS = (1e-3, 0.4, 37.5)            # fixed values of the by-value tests: the first rung, a mid-ladder value, a value far above every weight
SWEEP_FIELDS = pc.STEP_FIELDS["sweep"]
MARGIN_BELOW, MARGIN_ABOVE = 0.8, 1.25


def ladder(opt, start=0.0):
    """The reg values backward_sweep_regularized tries, in order: `start`, then max(reg x update_regularization, 1e-3) until one exceeds 1e2."""
    out, reg = [float(start)], float(start)
    while True:
        reg = max(reg * opt.update_regularization, 1e-3)
        if reg > 1e2:
            return out
        out.append(reg)


def carried(accepted):
    """The reg the loop leaves for the next DDP iteration."""
    reg = accepted / 20
    return 0.0 if reg < 1e-6 else reg


def critical_reg(solver, b, rel=1e-9):
    """Smallest reg at which backward_sweep passes for problem b of a solver holding LQ data (bisection to `rel`); 0 if reg = 0 passes."""
    if solver.backward_sweep(0.0)[b]:
        return 0.0
    lo, hi = 0.0, 1e-3
    while not solver.backward_sweep(hi)[b]:
        lo, hi = hi, 2 * hi
        assert hi < 1e6, "no reg makes this sweep pass"
    while hi - lo > rel * hi:
        mid = 0.5 * (lo + hi)
        if solver.backward_sweep(mid)[b]:
            hi = mid
        else:
            lo = mid
    return hi


def critical_regs(solver, rel=1e-8):
    """critical_reg of every problem of the batch in one joint bisection (a sweep call runs the whole batch; the verdict is monotonic in reg)."""
    B = solver.batch
    ok = solver.backward_sweep(0.0).astype(bool)
    lo, hi = np.zeros(B), np.where(ok, 0.0, np.inf)
    top = 1e-3
    while np.isinf(hi).any():
        ok = solver.backward_sweep(top).astype(bool)
        hi = np.where(ok & (top < hi), top, hi); lo = np.where(~ok & (top > lo), top, lo)
        top *= 2
        assert top < 1e6, "no reg makes this sweep pass"
    while True:
        gap = np.where(hi > 0, (hi - lo) / np.maximum(hi, 1e-300), 0.0)
        b = int(np.argmax(gap))
        if gap[b] <= rel:
            return hi
        mid = 0.5 * (lo[b] + hi[b])
        ok = solver.backward_sweep(mid).astype(bool)
        hi = np.where(ok & (mid < hi), mid, hi); lo = np.where(~ok & (mid > lo), mid, lo)


def prepare(s, opt):
    """LQ data of the first iterate: what every sweep below runs on."""
    s.hybrid_rollout(0.0, opt); s.update_nominal_trajectory(); s.compute_cost(opt); s.LQ_approximation(opt)


def srb_x0(x0):
    return np.ascontiguousarray(x0[:, list(range(6)) + list(range(18, 24))])     # StateProjection (MHPCReset.h:24-26)


class Case:
    """A problem with negative control weights r on the phases `on` (None: all): Quu is indefinite at reg = 0."""

    def __init__(self, name, make, x0, setting, opt_kw, r, on=None):
        self.name, self._make, self._x0, self.setting, self.opt_kw, self.r, self.on = name, make, x0, setting, dict(opt_kw), r, on

    def phases(self, r=None):
        ph = self._make()
        for i, p in enumerate(ph):
            if self.on is None or i in self.on:
                for j in range(pkg._abi.MODEL_DIMS[p["desc"].model][1]):
                    p["desc"].r[j] = self.r if r is None else r
        return ph

    def x0(self, phases):
        return self._x0(phases)

    def opt(self, **kw):
        d = dict(self.opt_kw); d.update(kw)
        return self.setting(**d)

    def critical_expected(self, phases):
        return max(-self.r * phases[i]["desc"].dt for i in range(len(phases)) if self.on is None or i in self.on)

    def solver(self, lib, phases=None, **kw):
        ph = self.phases() if phases is None else phases
        return pc.make_pair(pkg, lib, lib, ph, self.x0(ph), **kw)[0]


def indefinite_cases():
    P = pkg.problems
    wb = dict(ReB_active=0)
    return [
        Case("stance", lambda: P.wb_stance_problem(horizon=6), lambda ph: P.wb_ensemble_x0(2, 9), pkg.mhpc_ddp_setting, wb, -32.4),
        # fails in phase 2, after phase 3 has been swept and before phases 1 and 0
        Case("trot_mid", lambda: P.wb_trot_problem(horizons=(4, 3, 3, 3)), lambda ph: P.wb_ensemble_x0(2, 20241222), pkg.mhpc_ddp_setting, wb, -32.4, on=(2,)),
        Case("mhpc_tail", lambda: P.mhpc_problem(wb_horizons=(4, 3), srb_horizons=(3, 2)), lambda ph: P.wb_ensemble_x0(2, 20241222), pkg.mhpc_ddp_setting, wb, -0.06, on=(3,)),
        Case("hkd", lambda: P.hkd_trot_problem(horizons=(3, 4, 3, 3)), lambda ph: P.hkd_ensemble_x0(2, 11, ph), P.hkd_ddp_setting, {}, -0.31, on=(1,)),
    ]


def case_by_name(name):
    return {c.name: c for c in indefinite_cases()}[name]


def _rungs(lad, crit, tag):
    """Index of the accepted rung of `lad` for the critical value, after the margin check (a condition on the INPUT: change r, never the bound)."""
    idx = next(i for i, v in enumerate(lad) if v >= crit)
    assert idx >= 1, (tag, "reg = start already passes", lad[0], crit)
    below, above = lad[idx - 1], lad[idx]
    assert below <= MARGIN_BELOW * crit and above >= MARGIN_ABOVE * crit, f"{tag}: critical reg {crit:.6g} between rungs {below:.6g} / {above:.6g}: too close, change r"
    return idx


def expected_counts(case):
    """Rungs and n_reg_iters from the critical value -r dt alone (no sweep is run): what the device tests hold the retry loop to.  The host test
    of check_margins pins that the bisected critical values give the same numbers."""
    phases = case.phases(); opt = case.opt(); crit = case.critical_expected(phases)
    lad = ladder(opt); i1 = next(i for i, v in enumerate(lad) if v >= crit)
    lad2 = ladder(opt, carried(lad[i1])); i2 = next(i for i, v in enumerate(lad2) if v >= crit)
    return dict(rejected=lad[i1 - 1], accepted=lad[i1], n_reg_1=i1 + 1, rejected_2=lad2[i2 - 1], accepted_2=lad2[i2], n_reg_2=i1 + 1 + i2 + 1)


_MARGINS = {}


def check_margins(case, oracle_lib, oracle_ld_lib):
    """CPU only.  Asserts for every problem of the case: the fp64 and the long-double oracle agree on the critical reg to 1e-6 relative, and it
    sits clear of the ladder rungs (see the module docstring) in the first DDP iteration and, from the state a one-iteration solve leaves
    (hybrid_rollout(0) -> compute_cost -> LQ_approximation on the solved handle), in the second, whose ladder starts at accepted / 20.
    Returns rejected / accepted reg and n_reg_iters of the first search and of both (memoised: several tests need the numbers)."""
    if case.name in _MARGINS:
        return _MARGINS[case.name]
    phases = case.phases(); opt = case.opt(); batch = case.x0(phases).shape[0]
    out = None
    so, sx = case.solver(oracle_lib, phases), case.solver(oracle_ld_lib, phases)
    for s in (so, sx):
        prepare(s, opt)
    first = []
    cs, cxs = critical_regs(so), critical_regs(sx)
    for b in range(batch):
        c, cx = cs[b], cxs[b]
        assert abs(c - cx) <= 1e-6 * cx, (case.name, b, c, cx)
        assert abs(c - case.critical_expected(phases)) <= 1e-3 * c, (case.name, b, c)      # -r dt: the input is what its description says
        lad = ladder(opt); idx = _rungs(lad, c, f"{case.name}[{b}] first")
        first.append((lad[idx - 1], lad[idx], idx + 1, c))
    assert len({f[:3] for f in first}) == 1, first
    rejected, accepted, n1, _ = first[0]
    so.close(); sx.close()
    # second iteration, from a fresh pair of handles
    so, sx = case.solver(oracle_lib, phases), case.solver(oracle_ld_lib, phases)
    o1 = case.opt(max_AL_iter=1, max_DDP_iter=1)
    second = []
    for s in (so, sx):
        s.solve(o1)
        assert (s.info_arrays()["n_reg_iters"] == n1).all() and (s.info_arrays()["status"] == 0).all(), s.info_arrays()
        s.hybrid_rollout(0.0, opt); s.compute_cost(opt); s.LQ_approximation(opt)
    cs, cxs = critical_regs(so), critical_regs(sx)
    for b in range(batch):
        c, cx = cs[b], cxs[b]
        assert abs(c - cx) <= 1e-6 * cx, (case.name, b, c, cx)
        lad = ladder(opt, carried(accepted)); idx = _rungs(lad, c, f"{case.name}[{b}] second")
        second.append((lad[idx - 1], lad[idx], idx + 1, c))
    assert len({f[:3] for f in second}) == 1, second
    so.close(); sx.close()
    out = dict(rejected=rejected, accepted=accepted, n_reg_1=n1, critical=[float(f[3]) for f in first],
               rejected_2=second[0][0], accepted_2=second[0][1], n_reg_2=n1 + second[0][2], critical_2=[float(f[3]) for f in second])
    _MARGINS[case.name] = out
    return out


def fixed_problem(name, batch=2):
    """The well-posed problems of the fixed-reg comparisons: (phases, x0, option)."""
    P = pkg.problems
    opt = pkg.mhpc_ddp_setting()
    x0 = P.wb_ensemble_x0(batch, 20241222)
    if name == "stance":
        return P.wb_stance_problem(horizon=5), x0, opt
    if name == "trot":
        return P.wb_trot_problem(horizons=(4, 3, 3, 3)), x0, opt
    if name == "trot_ss":          # option.MS = 0: single shooting, no defects
        return P.wb_trot_problem(horizons=(4, 3, 3, 3)), P.wb_ensemble_x0(batch, 20241227), pkg.mhpc_ddp_setting(MS=0)
    if name == "mhpc":             # 36 -> 12 across the impact reset
        return P.mhpc_problem(wb_horizons=(4, 3), srb_horizons=(3, 2)), x0, opt
    if name == "srb_only":
        return P.mhpc_problem(wb_schedule=(), wb_horizons=(), srb_horizons=(4, 3)), srb_x0(x0), opt
    if name == "hkd":
        ph = P.hkd_trot_problem(horizons=(3, 4, 3, 3))
        return ph, P.hkd_ensemble_x0(batch, 11, ph), P.hkd_ddp_setting()
    if name == "flight":           # stance -> flight -> four-foot touchdown
        return P.wb_trot_problem(schedule=((1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1)), horizons=(3, 3, 3), last_next=(1, 1, 1, 1)), P.wb_ensemble_x0(batch, 31), opt
    if name == "single_knot":      # one knot per phase, one problem
        return P.wb_trot_problem(schedule=((0, 1, 1, 0), (1, 0, 0, 1)), horizons=(1, 1), last_next=(0, 1, 1, 0)), P.wb_ensemble_x0(1, 77), opt
    raise KeyError(name)


FIXED_PROBLEMS = ("stance", "trot", "mhpc", "srb_only", "hkd", "flight", "single_knot", "trot_ss")


def compare_sweep(sa, sb, nph, opt, tag, fields=None):
    """After backward_sweep(reg) on both (sa: fp64 oracle): the sweep fields at 1e-8 x scale (K 1e-6 absolute), both expected cost changes at
    1e-8, then linear_rollout(1.0) on both, DX at 1e-8 x scale and the cost changes again.  The plain tolerances: no arbiter.
    Returns the worst error over scale (for K: over max(1, |K|)) of the fields."""
    rep = pc.compare(sa, sb, fields or SWEEP_FIELDS, nph, 1e-8, tag, atol_K=1e-6)

    def dv(where):
        da, db = sa.get_exp_cost_change(), sb.get_exp_cost_change()
        for q in (0, 1):
            assert np.allclose(da[q], db[q], rtol=1e-8, atol=1e-10), (tag, where, q, da[q], db[q])
    dv("sweep")
    for s in (sa, sb):
        s.linear_rollout(1.0, opt)
    rep.update(pc.compare(sa, sb, ["DX"], nph, 1e-8, tag))
    dv("linear")
    worst = max(v[0] / v[1] for v in rep.values())
    print(f"[reg] {tag}: worst error / scale {worst:.2e}, worst |dK| {max([v[0] for k, v in rep.items() if k[0] == 'K'], default=0.0):.2e}")
    return worst


def fields_equal(sa, sb, nph, fields=None):
    """Bit-identical fields on two handles."""
    for f in fields or SWEEP_FIELDS:
        for i in range(nph):
            a, b = sa.field(i, f), sb.field(i, f)
            assert np.array_equal(a, b), (f, i, float(np.abs(a - b).max()))


def numpy_sweep(s, reg=0.0, dtype=np.float64):
    """SinglePhase::backward_sweep (SinglePhase.cpp:323-391) in numpy over the LQ data of a ONE-phase solver, any (n, m, p), problem 0, in `dtype`.
    Returns K, dU, dV, the stored Quu and H[0]."""
    assert len(s.phases) == 1
    n, m, p = s.dims[0]
    g = lambda f: s.field(0, f)[0].astype(dtype)
    A, B, lx, lu, lxx, luu, lux, Df = g("A"), g("B"), g("LX"), g("LU"), g("LXX"), g("LUU"), g("LUX"), g("DEFECT")
    if p:
        C, D, ly, lyy = g("C"), g("D"), g("LY"), g("LYY")
    G = g("PHIX")[0].copy(); H = g("PHIXX")[0].copy()
    h = A.shape[0]; Ks = np.zeros((h, m, n), dtype); dUs = np.zeros((h, m), dtype); Quus = np.zeros((h, m, m), dtype); dV = dtype(0)
    In, Im = np.eye(n, dtype=dtype), np.eye(m, dtype=dtype)
    for k in range(h - 1, -1, -1):
        Gn = G + H @ Df[k + 1]
        Qx = lx[k] + A[k].T @ Gn; Qu = lu[k] + B[k].T @ Gn
        Qxx = lxx[k] + A[k].T @ H @ A[k]; Quu = luu[k] + B[k].T @ H @ B[k]; Qux = lux[k] + B[k].T @ H @ A[k]
        if p:
            Qx = Qx + C[k].T @ ly[k]; Qu = Qu + D[k].T @ ly[k]
            Qxx = Qxx + C[k].T @ lyy[k] @ C[k]; Quu = Quu + D[k].T @ lyy[k] @ D[k]; Qux = Qux + D[k].T @ lyy[k] @ C[k]
        Qxx = Qxx + dtype(reg) * In; Quu = Quu + dtype(reg) * Im
        Quus[k] = Quu
        Qi = np.linalg.inv(Quu - dtype(1e-9) * Im).astype(dtype)
        Qxx = (Qxx + Qxx.T) / 2
        dUs[k] = -Qi @ Qu; Ks[k] = -Qi @ Qux
        G = Qx - Qux.T @ (Qi @ Qu); H = Qxx - Qux.T @ (Qi @ Qux)
        dV += Qu @ dUs[k]
    return Ks, dUs, dV, Quus, H
