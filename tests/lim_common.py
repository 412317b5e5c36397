"""Shared by tests/test_limits_host.py and tests/test_limits_gpu.py: per-problem constraint limits (include/hsddp_limits.h).

The reference.  The oracle has no per-problem limits, so a batch of B problems with limit rows is held against B SINGLE-problem handles of
liboracle_hsddp.so whose descriptors carry problem b's limits (whole-body phases only, the entries that are not NaN): LimitedOracle is
pw_common.StackedOracle with those descriptors - and, for the combination tests, the cost-weight products and touchdown heights as well.

The inputs.  barrier_common.WB_SCHEDULE (horizons 2, 3, 2) with every constraint family on (phases(): the joint-speed constraint switched on, the
joint box of barrier_common widened by 0.5 rad, wide speed and height limits, a Reb per group), the shared nominal trajectory of problems.wb_trot_problem, ensemble initial
states.  Under multiple shooting every knot of the first iterate starts from the shared Xbar[k] (knot 0 of phase 0: from x0), so the LIMITS decide
the region of the barrier a problem's constraints sit in: limit_rows() puts

  box families and height   limit = nominal value -+ an offset: OFFSETS[family][region] is the value g of the tightest constraint of the family at
                            a nominal knot - above the group's delta, inside [0, delta] or violated, each by far more than MARGIN;
  pyramid                   mu_b from the largest ratio max(|fx|, |fy|) / fz over the contact feet and knots of problem b's own forces in an oracle
                            run without limits (forces()): that ratio plus a margin is inside, 0.5 x it is violated, 0.45 (the descriptor has 0.6) above.

Row 0 is all NaN.  Row b >= 1, k = b - 1: k % 4 in (0, 1) sets every entry, family f (torque, jointspeed, joint, height, grf) in region (k + f) % 3;
k % 4 == 2 sets mu alone and k % 4 == 3 torque_limit alone, region (k // 4) % 3 - the NaN fallback per entry.  coverage() holds the outcome.

The emulator.  LimEmu runs the host build of the programs with limits (tests/_emu/lim_emu.cpp) behind the Solver interface.
"""
import ctypes as C

import numpy as np

import barrier_common as bc
import pw_common as pw
import walk_ref as wr
from conftest import pkg

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
WAVE, QUAD = pw.WAVE, pw.QUAD
ROW = 12
TORQUE, JLB, JUB, HMIN, MU, JSLB, JSUB, PAD = 0, 1, 4, 7, 8, 9, 10, 11
MODEL_WB = 0
BATCHES = (1, 5, 17)
SEED = bc.SEED
FAMILIES = ("torque", "jointspeed", "joint", "height", "grf")
REB = dict(torque=(0.125, 0.125, 0.1), jointspeed=(0.25, 0.25, 0.1), joint=(0.0625, 0.0625, 0.1), minheight=(0.03125, 0.03125, 0.1), grf=(0.5, 0.5, 0.3))
# g of the family's tightest constraint at a nominal knot, by region (above, inside, violated); the deltas are REB's first entries
OFFSETS = dict(torque=(5.0, 0.06, -0.3), jointspeed=(2.0, 0.1, -0.2), joint=(0.2, 0.03, -0.1), height=(0.08, 0.012, -0.02))
MU_ABOVE, MU_INSIDE_G, MU_VIOLATED = 0.45, 0.2, 0.5      # inside: the tightest pyramid row at g = 0.2 N (delta 0.5); violated: half the ratio


def phases():
    """WB_SCHEDULE with every constraint family on; the descriptor's limits are wide: every constraint of the shared nominal is above its delta."""
    ph = pkg.problems.wb_trot_problem(**bc.WB_SCHEDULE)
    for p in ph:
        d = p["desc"]
        d.c_torque = d.c_joint = d.c_minheight = d.c_grf = d.c_jointspeed = 1
        for i in range(3):
            d.joint_lb[i], d.joint_ub[i] = bc.JOINT_LB[i] - 0.5, bc.JOINT_UB[i] + 0.5
        d.jointspeed_lb, d.jointspeed_ub = -8.0, 8.0
        d.h_min = pkg.problems.Z_NOM - 0.15
        for k, v in REB.items():
            setattr(d, "reb_" + k, bc.Reb(*v))
    return ph


def x0_of(batch):
    return pkg.problems.wb_ensemble_x0(batch, SEED)


def limited_phases(phases, row):
    """The phase list with the row's entries (those that are not NaN) in the descriptors of its whole-body phases; everything else is shared."""
    out = []
    for p in phases:
        q = dict(p)
        d = type(p["desc"]).from_buffer_copy(p["desc"])
        if d.model == MODEL_WB:
            if not np.isnan(row[TORQUE]): d.torque_limit = float(row[TORQUE])
            for j in range(3):
                if not np.isnan(row[JLB + j]): d.joint_lb[j] = float(row[JLB + j])
                if not np.isnan(row[JUB + j]): d.joint_ub[j] = float(row[JUB + j])
            if not np.isnan(row[HMIN]): d.h_min = float(row[HMIN])
            if not np.isnan(row[MU]): d.mu = float(row[MU])
            if not np.isnan(row[JSLB]): d.jointspeed_lb = float(row[JSLB])
            if not np.isnan(row[JSUB]): d.jointspeed_ub = float(row[JSUB])
        q["desc"] = d
        out.append(q)
    return out


def desc_row(d):
    return np.array([d.torque_limit, *d.joint_lb[:3], *d.joint_ub[:3], d.h_min, d.mu, d.jointspeed_lb, d.jointspeed_ub, 0.0])


def resolved(phases, rows):
    """[nph, B, 12]: what problem b uses in phase i - numpy's statement of k_pack_limits."""
    return np.stack([np.where(np.isnan(rows), desc_row(p["desc"])[None, :], rows) for p in phases])


class LimitedOracle(pw.StackedOracle):
    """B single-problem handles whose descriptors carry problem b's limits (and scale rows / touchdown heights, if given)."""

    def __init__(self, lib, phases, x0, rows, scales=None, heights=None):
        self.batch = x0.shape[0]
        self.phases = phases
        self.rows = rows
        self.scales = scales
        self.s = []
        for b in range(self.batch):
            ph = self.descriptors(phases, b)
            for i, hts in (heights or {}).items():
                assert np.all(hts[b] == hts[b][0])
                ph[i]["desc"].ground_height = float(hts[b][0])
            s = pkg.Solver(lib, ph, batch=1)
            for i, p in enumerate(ph):
                X, U = np.asarray(p["Xbar"]), np.asarray(p["Ubar"])
                s.set_nominal(i, X[b:b + 1] if X.ndim == 3 else X, U[b:b + 1] if U.ndim == 3 else U)
            s.set_initial_condition(np.ascontiguousarray(x0[b:b + 1]))
            self.s.append(s)

    def descriptors(self, phases, b):
        ph = limited_phases(phases, self.rows[b])
        return ph if self.scales is None else pw.scaled_phases(ph, self.scales[b])

    def reconfigure(self, phases, src, shift):
        for b, s in enumerate(self.s):
            s.reconfigure(self.descriptors(phases, b), src, shift)
        self.phases = phases


def forces(oracle_lib, phases, x0):
    """Y per phase [B, h, 12] of the first rollout of an oracle run WITHOUT limits (eps = 0: the nominal trajectory from each problem's x0)."""
    s = pw.StackedOracle(oracle_lib, phases, x0, np.ones((x0.shape[0], pw.ROW)))
    s.hybrid_rollout(0.0, pkg.mhpc_ddp_setting())
    Y = [s.field(i, "Y").copy() for i in range(len(phases))]
    s.close()
    return Y


def _tightest_ratio(phases, Y, b):
    """(ratio, fz) of the contact foot and knot of problem b with the largest max(|fx|, |fy|) / fz."""
    best = (0.0, 1.0)
    for p, y in zip(phases, Y):
        for l in range(4):
            if p["desc"].contact[l] > 0:
                f = y[b, :, 3 * l:3 * l + 3]
                for k in range(f.shape[0]):
                    r = max(abs(f[k, 0]), abs(f[k, 1])) / f[k, 2]
                    if r > best[0]:
                        best = (r, f[k, 2])
    return best


def limit_rows(batch, phases, Y):
    """[B, 12], NaN where unset; see the module's docstring.  Y: forces() of the same problems."""
    xn, un = np.asarray(phases[0]["Xbar"])[0], np.concatenate([np.asarray(p["Ubar"]) for p in phases])
    umax = float(np.abs(un).max()); q = xn[6:9]; z = float(xn[2])
    assert np.allclose(np.asarray(phases[0]["Xbar"])[:, 24:36], 0.0) and np.allclose(np.tile(q, 4), xn[6:18])      # the nominal: one leg pose, joints at rest
    rows = np.full((batch, ROW), np.nan)
    for b in range(1, batch):
        k = b - 1
        full = k % 4 in (0, 1)
        reg = {f: (k + i) % 3 if full else (k // 4) % 3 for i, f in enumerate(FAMILIES)}
        if full or k % 4 == 3:
            rows[b, TORQUE] = umax + OFFSETS["torque"][reg["torque"]]
        if full or k % 4 == 2:
            ratio, fz = _tightest_ratio(phases, Y, b)
            rows[b, MU] = (MU_ABOVE, ratio + MU_INSIDE_G / fz, MU_VIOLATED * ratio)[reg["grf"]]
        if full:
            o = OFFSETS["jointspeed"][reg["jointspeed"]]; rows[b, JSLB], rows[b, JSUB] = -o, 2.0
            o = OFFSETS["joint"][reg["joint"]]; rows[b, JLB:JLB + 3] = q - o; rows[b, JUB:JUB + 3] = q + 0.4
            rows[b, HMIN] = z - OFFSETS["height"][reg["height"]]
    return rows


def coverage(phases, rows, X, U, Y, D):
    """{(family, region): [(b, phase, knot, constraint)]} of each problem's constraint values under ITS OWN limits (barrier_common.constraint_values on
    the limited descriptors) against the deltas D, MARGIN to both branch points - counted only where the value is `above` under the DESCRIPTOR's
    limits, so that the region is the limit's doing."""
    cells = {}
    for i, p in enumerate(phases):
        lay = bc.layout(p["desc"])
        for b in range(rows.shape[0]):
            d = limited_phases([p], rows[b])[0]["desc"]
            g = bc.constraint_values(d, X[i][b], U[i][b], Y[i][b]); g0 = bc.constraint_values(p["desc"], X[i][b], U[i][b], Y[i][b])
            for k in range(g.shape[0]):
                for c, (fam, _, _) in enumerate(lay):
                    dl = D[i][b, k, c]
                    if bc.has_margin(g[k, c], dl) and bc.has_margin(g0[k, c], dl) and bc.region(g0[k, c], dl) == "above":
                        cells.setdefault((fam, bc.region(g[k, c], dl)), []).append((b, i, k, c))
    return cells


def build_emu(tmpdir):
    raw = wr.build_so(tmpdir, "lim_emu.cpp", "libhsddp_lim_emu.so")
    raw.lim_emu_hybrid_rollout.argtypes = [C.c_void_p, C.c_double, C.c_void_p, DP, DP, C.c_int]
    raw.lim_emu_LQ_approximation.argtypes = [C.c_void_p, C.c_void_p, DP, DP]
    raw.lim_emu_pack.argtypes = [DP, DP, DP, C.c_int, C.c_int, DP, C.c_int, C.c_int, C.c_int]
    raw.lim_emu_friction.argtypes = [DP, DP, C.c_int, C.c_int, DP, IP, C.c_int, C.c_double]
    raw.lim_emu_desc_rows.argtypes = [C.c_void_p, DP]
    raw.lim_emu_check_set.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    raw.lim_emu_check_get.argtypes = [C.c_int] * 6
    raw.lim_emu_check_kappa.argtypes = [C.c_double]
    return pkg._abi.bind(raw), raw


class LimEmu:
    """A batch-B handle of the lane emulator whose rollout and LQ steps run the programs with limits (rows [B, 12], None: the programs without the
    switch) and, optionally, scales [B, 84].  Everything else is the emulator's Solver."""

    def __init__(self, lib, raw, phases, x0, rows, program, scales=None):
        self.raw, self.program = raw, program
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
        self.scales = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
        self.s = pkg.Solver(lib, phases, batch=x0.shape[0])
        for i, p in enumerate(phases):
            self.s.set_nominal(i, p["Xbar"], p["Ubar"])
        self.s.set_initial_condition(x0)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(DP)

    def hybrid_rollout(self, eps, opt):
        assert self.raw.lim_emu_hybrid_rollout(self.s.h, float(eps), C.byref(opt), self._p(self.scales), self._p(self.rows), self.program) == 0

    def LQ_approximation(self, opt):
        assert self.raw.lim_emu_LQ_approximation(self.s.h, C.byref(opt), self._p(self.scales), self._p(self.rows)) == 0

    def __getattr__(self, name):
        return getattr(self.s, name)


def row_kwargs(rows):
    """Solver.set_limits' keyword arguments for rows [nb, 12]."""
    return dict(torque_limit=rows[:, TORQUE], joint_lb=rows[:, JLB:JLB + 3], joint_ub=rows[:, JUB:JUB + 3], h_min=rows[:, HMIN], mu=rows[:, MU],
                jointspeed_lb=rows[:, JSLB], jointspeed_ub=rows[:, JSUB])


def rows_of(lim):
    """[nb, 12] from the dict Solver.limits returns (pad 0)."""
    nb = lim["mu"].shape[0]
    out = np.zeros((nb, ROW))
    for n, (o, w) in pkg._abi.LIMITS_FIELDS.items():
        out[:, o:o + w] = lim[n].reshape(nb, w)
    return out


def make_hip(hip_lib, phases, x0, rows=None, scales=None, **kw):
    """A batch-B handle of libhsddp_hip.so with the rows set through Solver.set_limits (and scales through set_weight_scales)."""
    s = pkg.Solver(hip_lib, phases, batch=x0.shape[0], **kw)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    if scales is not None:
        s.set_weight_scales(*pw.split(scales))
    if rows is not None:
        s.set_limits(**row_kwargs(rows))
    return s


def simple_rows(batch):
    """Rows for any window: row 0 all NaN, the others a torque limit of 9 .. 14 Nm and a friction coefficient of 0.3 .. 0.5 of their own, every second
    one a joint-speed box as well."""
    rows = np.full((batch, ROW), np.nan)
    if batch > 1:
        rows[1:, TORQUE] = np.linspace(9.0, 14.0, batch - 1); rows[1:, MU] = np.linspace(0.3, 0.5, batch - 1)
        rows[2::2, JSLB] = -6.0; rows[2::2, JSUB] = 7.0
    return rows
