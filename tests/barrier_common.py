"""Shared by tests/test_barrier_host.py and tests/test_barrier_gpu.py: inputs that put the relaxed log barrier of every inequality family on
both of its branches (-log g above delta, the quadratic extension at or below it), and solves in which the update of eps / delta / sigma /
lambda between augmented-Lagrangian iterations does something.

The constraint values g are no field of the ABI; constraint_values() states them in numpy from X, U and Y, in the kernels' order
(include/hsddp.h: torque 24, joint speed 24 if present, joint 24, height 1, then 5 rows per contact foot in rank order; SRB: height; HKD: 5 rows
per contact leg from u[0:12], legs FR FL HR HL).  Rows of a foot: fz, mu fz - fx, mu fz + fx, mu fz - fy, mu fz + fy.

Regions of a value against its delta: above (g > delta), inside (0 <= g <= delta), violated (g < 0).  A value counts for a coverage cell only
with MARGIN to both branch points, so rounding cannot move it across a branch between backends.

Step cases (per iterate, parity_common.run_steps).  Every knot of every phase starts from a per-problem Xbar / Ubar (multiple shooting restarts
each knot from Xbar, and the lane-quad wave holds 16 knots of several problems), so the limits are met at every knot of the first iterate:

  wb_edges      schedule (1111, 0110, 1001), horizons (2, 3, 2), tightened limits; for joint j of problem b, (b + j + off) % 3 picks the region and
                ((b + j + off) // 3) % 2 the half (lower / upper bound), off = 0 / 2 / 4 for torque / joint / joint speed: over six problems every
                joint meets all six combinations in all three families.  The height cycles through its regions.  Every seventh problem is the
                plain ensemble state: its lanes sit above delta beside lanes that do not (the wave-wide shortcut of q_barrier with mixed lanes).
  wb_grf_edges  the same schedule, mu = 0.1 and per-knot torque offsets (a fixed SplitMix64 stream): pyramid rows inside and violated.
  hkd_edges     hkd_trot_problem (3, 4, 3, 3): per-problem, per-knot forces put one row of each contact leg inside or violated, in turn.
  srb_edges     the SRB tail (4, 3): the base height above, inside and below h_min over the problems.

Update cases (full solves with update_ReB = 7, update_relax = 0.5, max_DDP_iter = 2, max_AL_iter = 1 .. 4): wb_updates, hkd_updates, srb_updates -
limits that stay violated, a (delta, delta_min, eps) of its own per group with delta / delta_min no power of two in some groups (the floor
clamps to a value the multiplication alone does not reach), a sigma_max low enough to be hit."""
import numpy as np

from conftest import pkg

P = pkg.problems
Reb, Al = pkg._abi.Reb, pkg._abi.Al
SEED = 20241222
MARGIN = 1e-3
REGIONS = ("above", "inside", "violated")
STEP_CASES = ("wb_edges", "wb_grf_edges", "hkd_edges", "srb_edges")
UPDATE_CASES = ("wb_updates", "hkd_updates", "srb_updates")
AL_ITERS = (1, 2, 3, 4)
PARAM_FIELDS = ("REB_EPS", "REB_DELTA", "AL_SIGMA", "AL_LAMBDA")
UPDATE_REB, UPDATE_RELAX = 7.0, 0.5

WB_SCHEDULE = dict(schedule=((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1)), horizons=(2, 3, 2), last_next=(1, 1, 1, 1))
JOINT_LB, JOINT_UB = (-0.25, -1.25, 1.75), (0.25, -0.75, 2.25)      # +-0.25 around the nominal pose (0, -1, 2)
SPEED_LIMIT = 3.0
TORQUE_LIMIT = 17.0
INSIDE = 0.05                                                       # distance inside a limit of the `inside` entries; every delta of these families is above it
FAMILY_OFFSET = dict(torque=0, joint=2, jointspeed=4)
# wb_grf_edges: the pyramid cells no qualifying input reaches (row, region); listed in DESIGN.md as well.  None.
GRF_UNCOVERED = ()


# ------------------------------------------------------------------------------------------------------------- the constraints in numpy
def layout(desc):
    """[(family, index within family, group)] of the path constraints of a phase, in the kernels' order.  The whole-body pyramid is indexed
    5 x rank + row (rank of the foot among the contact feet), the kinodynamic one 5 x leg + row."""
    out = []
    contact = [l for l in range(4) if desc.contact[l] > 0]
    if desc.model == pkg.MODEL_WB:
        if desc.c_torque:
            out += [("torque", i, "torque") for i in range(24)]
        if desc.c_jointspeed:
            out += [("jointspeed", i, "jointspeed") for i in range(24)]
        if desc.c_joint:
            out += [("joint", i, "joint") for i in range(24)]
        if desc.c_minheight:
            out.append(("height", 0, "minheight"))
        if desc.c_grf:
            out += [("grf", 5 * rank + r, "grf") for rank in range(len(contact)) for r in range(5)]
    elif desc.model == pkg.MODEL_SRB:
        if desc.c_minheight:
            out.append(("height", 0, "minheight"))
    else:
        if desc.c_grf:
            out += [("pyramid", 5 * l + r, "grf") for l in contact for r in range(5)]
    return out


def group_params(desc, group):
    """The Reb (delta, delta_min, eps) a group starts from."""
    return getattr(desc, "reb_" + group)


def _pyramid(f, mu):
    """f [..., 3] -> the 5 rows [..., 5]."""
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([fz, mu * fz - fx, mu * fz + fx, mu * fz - fy, mu * fz + fy], axis=-1)


def constraint_values(desc, X, U, Y=None):
    """g [..., h, ng] of the knots 0 .. h - 1 of one phase from X [..., >= h, n], U [..., h, m] and, whole body, the contact forces Y [..., h, 12]."""
    h = desc.horizon
    X, U = np.asarray(X)[..., :h, :], np.asarray(U)[..., :h, :]
    contact = [l for l in range(4) if desc.contact[l] > 0]
    cols = []
    if desc.model == pkg.MODEL_WB:
        if desc.c_torque:
            cols += [desc.torque_limit - U, U + desc.torque_limit]
        if desc.c_jointspeed:
            cols += [X[..., 24:36] - desc.jointspeed_lb, desc.jointspeed_ub - X[..., 24:36]]
        if desc.c_joint:
            lb, ub = np.tile(np.array(desc.joint_lb[:]), 4), np.tile(np.array(desc.joint_ub[:]), 4)
            cols += [X[..., 6:18] - lb, ub - X[..., 6:18]]
        if desc.c_minheight:
            cols.append(X[..., 2:3] - desc.h_min)
        if desc.c_grf:
            Y = np.asarray(Y)[..., :h, :]
            cols += [_pyramid(Y[..., 3 * l:3 * l + 3], desc.mu) for l in contact]
    elif desc.model == pkg.MODEL_SRB:
        if desc.c_minheight:
            cols.append(X[..., 2:3] - desc.h_min)
    else:
        if desc.c_grf:
            cols += [_pyramid(U[..., 3 * l:3 * l + 3], desc.mu) for l in contact]
    if not cols:
        return np.zeros(U.shape[:-1] + (0,))
    return np.concatenate(cols, axis=-1)


def region(g, delta):
    """'above' (g > delta), 'inside' (0 <= g <= delta) or 'violated' (g < 0): the branch of the barrier and, in a solve, of the update."""
    if g > delta:
        return "above"
    return "inside" if g >= 0 else "violated"


def has_margin(g, delta, margin=MARGIN):
    return abs(g) >= margin and abs(g - delta) >= margin


def coverage(phases, G, D, margin=MARGIN):
    """{(family, index, region): [(problem, (phase, knot)), ...]} over the window.  phases: phase dicts; G, D: per phase the constraint values and
    the deltas, each [B, h, ng].  Values without `margin` to 0 and to delta count for no cell."""
    cells = {}
    for i, p in enumerate(phases):
        lay = layout(p["desc"])
        g, d = np.asarray(G[i]), np.asarray(D[i])
        assert g.shape == d.shape and g.shape[2] == len(lay), (i, g.shape, d.shape, len(lay))
        for b in range(g.shape[0]):
            for k in range(g.shape[1]):
                for c, (fam, idx, _) in enumerate(lay):
                    if has_margin(g[b, k, c], d[b, k, c], margin):
                        cells.setdefault((fam, idx, region(g[b, k, c], d[b, k, c])), []).append((b, (i, k)))
    return cells


def oracle_constraints(s):
    """(G, D) per phase from a handle's X, U, Y and REB_DELTA fields."""
    G, D = [], []
    for i, p in enumerate(s.phases):
        y = s.field(i, "Y") if s.dims[i][2] else None
        G.append(constraint_values(p["desc"], s.field(i, "X"), s.field(i, "U"), y))
        D.append(s.field(i, "REB_DELTA"))
    return G, D


# ------------------------------------------------------------------------------------------------------------- step cases
def _per_problem(phases, X, U):
    """Per-problem nominal trajectories in the phase dicts: parity_common.make_pair and MultiPhaseDDP hand a 3-d Xbar to hsddp_set_nominal with
    per_problem = 1 (Solver.set_nominal)."""
    for p, x, u in zip(phases, X, U):
        p["Xbar"], p["Ubar"] = np.ascontiguousarray(x), np.ascontiguousarray(u)
    return phases


def _tighten(d, reb):
    """The tightened whole-body limits and a Reb per group."""
    for i in range(3):
        d.joint_lb[i], d.joint_ub[i] = JOINT_LB[i], JOINT_UB[i]
    d.c_jointspeed, d.jointspeed_lb, d.jointspeed_ub = 1, -SPEED_LIMIT, SPEED_LIMIT
    d.h_min = P.Z_NOM - 0.02
    for k, v in reb.items():
        setattr(d, "reb_" + k, Reb(*v))


def _outside(b, j):
    """0.07 .. 0.3, in five steps over (problem, joint)."""
    return 0.07 + 0.23 * ((5 * b + j) % 5) / 4.0


def wb_edge_state(b, x_plain, u_plain):
    """(x, u) of edge problem b from its plain ensemble state and gravity-compensation torque."""
    x, u = x_plain.copy(), u_plain.copy()
    for j in range(12):
        def pick(fam):
            s = b + j + FAMILY_OFFSET[fam]
            return s % 3, (s // 3) % 2
        r, half = pick("joint")
        lb, ub = JOINT_LB[j % 3], JOINT_UB[j % 3]
        if r == 1:
            x[6 + j] = lb + INSIDE if half == 0 else ub - INSIDE
        elif r == 2:
            x[6 + j] = lb - _outside(b, j) if half == 0 else ub + _outside(b, j)
        r, half = pick("jointspeed")
        if r == 1:
            x[24 + j] = (-SPEED_LIMIT + INSIDE) if half == 0 else (SPEED_LIMIT - INSIDE)
        elif r == 2:
            x[24 + j] = -(SPEED_LIMIT + _outside(b, j + 1)) if half == 0 else SPEED_LIMIT + _outside(b, j + 1)
        r, half = pick("torque")                      # rows 0 - 11 hold the upper bound (limit - u), rows 12 - 23 the lower one
        if r == 1:
            u[j] = (TORQUE_LIMIT - INSIDE) if half == 0 else -(TORQUE_LIMIT - INSIDE)
        elif r == 2:
            u[j] = (TORQUE_LIMIT + 0.3) if half == 0 else -(TORQUE_LIMIT + 0.3)
    x[2] = P.Z_NOM - 0.02 + (0.05, 0.01, -0.02)[b % 3]          # height: above, inside, violated against delta = 2^-5
    return x, u


WB_EDGE_REB = dict(torque=(0.125, 0.125, 0.1), jointspeed=(0.25, 0.25, 0.1), joint=(0.0625, 0.0625, 0.1), minheight=(0.03125, 0.03125, 0.1), grf=(0.5, 0.5, 0.3))


def wb_edges(batch=7, reb=None, window=None):
    """(phases, x0).  Problems b with b % 7 == 6 are plain ensemble states (z raised to h_min + 0.04: above); the others are edge problems, numbered
    b - b // 7 so that any six consecutive ones hold all combinations.  window: another schedule than WB_SCHEDULE (the shifted window)."""
    phases = P.wb_trot_problem(**(window or WB_SCHEDULE))
    for p in phases:
        _tighten(p["desc"], reb or WB_EDGE_REB)
    plain = P.wb_ensemble_x0(batch, SEED)
    x0 = plain.copy()
    U = [np.tile(p["Ubar"][None], (batch, 1, 1)) for p in phases]
    for b in range(batch):
        if b % 7 == 6:
            x0[b, 2] = P.Z_NOM + 0.02
            continue
        e = b - b // 7
        for i, p in enumerate(phases):
            x0[b], U[i][b, :] = wb_edge_state(e, plain[b], p["Ubar"][0])
    X = [np.tile(x0[:, None, :], (1, p["desc"].horizon + 1, 1)) for p in phases]
    return _per_problem(phases, X, U), x0


GRF_MU, GRF_SCALE, GRF_SEED = 0.1, 6.0, 7
WB_GRF_REB = dict(torque=(0.125, 0.125, 0.1), jointspeed=(0.25, 0.25, 0.1), joint=(0.0625, 0.0625, 0.1), minheight=(0.03125, 0.03125, 0.1), grf=(1.0, 1.0, 0.3))


def wb_grf_edges(batch=6, mu=GRF_MU, scale=GRF_SCALE, seed=GRF_SEED):
    """(phases, x0): plain ensemble states at every knot, a slippery ground (mu) and torque offsets of up to +-scale per joint, knot and problem on
    top of the gravity compensation: the contact forces of the first iterate are a function of (Xbar[k], Ubar[k]) alone, so every (problem, knot)
    is one draw of the pyramid rows.  mu, scale and seed were chosen with the oracle on the CPU; the coverage test holds the outcome."""
    phases = P.wb_trot_problem(**WB_SCHEDULE)
    for p in phases:
        d = p["desc"]
        d.mu = mu
        for k, v in WB_GRF_REB.items():
            setattr(d, "reb_" + k, Reb(*v))
    x0 = P.wb_ensemble_x0(batch, SEED)
    rng = P.SplitMix64(seed)
    X, U = [], []
    for p in phases:
        h = p["desc"].horizon
        off = np.array([rng.next() for _ in range(batch * h * 12)]).reshape(batch, h, 12)
        U.append(p["Ubar"][None] + scale * (2.0 * off - 1.0))
        X.append(np.tile(x0[:, None, :], (1, h + 1, 1)))
    return _per_problem(phases, X, U), x0


HKD_REB = (0.125, 0.125, 0.5)
HKD_BATCH = 4


def hkd_edge_force(t, mu, fz=20.0):
    """A leg's force that puts pyramid row t % 5 inside (t % 10 < 5) or violated."""
    r, viol = t % 5, (t % 10) >= 5
    if r == 0:
        f = -0.2 if viol else INSIDE
        return np.array([0.0, 0.0, f])
    lat = mu * fz + (0.3 if viol else -INSIDE)         # mu fz -+ lateral = -0.3 or 0.05
    f = np.array([0.0, 0.0, fz])
    f[0 if r in (1, 2) else 1] = lat if r in (1, 3) else -lat
    return f


def hkd_edges(batch=HKD_BATCH, horizons=(3, 4, 3, 3), reb=HKD_REB):
    """(phases, x0).  Contact leg l at the c-th contact knot of problem b takes target (b + 3 c + l) % 10 - five rows x (inside, violated); the rows
    a target leaves alone sit above (fz = 20 N, mu = 0.7)."""
    phases = P.hkd_trot_problem(horizons=horizons)
    x0 = P.hkd_ensemble_x0(batch, 13, phases)
    X, U = [], []
    seen = [0] * 4
    for p in phases:
        d = p["desc"]; d.reb_grf = Reb(*reb)
        u = np.tile(p["Ubar"][None], (batch, 1, 1))
        for k in range(d.horizon):
            for l in range(4):
                if d.contact[l]:
                    for b in range(batch):
                        u[b, k, 3 * l:3 * l + 3] = hkd_edge_force(b + 3 * seen[l] + l, d.mu)
                    seen[l] += 1
        U.append(u); X.append(np.tile(p["Xbar"][None], (batch, 1, 1)))
    return _per_problem(phases, X, U), x0


SRB_REB = (0.0078125, 0.0078125, 0.1)
SRB_HEIGHTS = (0.05, 0.004, -0.02)            # above, inside, violated against delta = 2^-7


def _srb_x0(batch):
    x = P.wb_ensemble_x0(batch, 20241230)
    return np.ascontiguousarray(x[:, list(range(6)) + list(range(18, 24))])     # StateProjection (MHPCReset.h:24-26)


def srb_edges(batch=3, reb=SRB_REB):
    phases = P.mhpc_problem(wb_schedule=(), wb_horizons=(), srb_horizons=(4, 3))
    x0 = _srb_x0(batch)
    X, U = [], []
    for p in phases:
        d = p["desc"]; d.reb_minheight = Reb(*reb)
        x = np.tile(p["Xbar"][None], (batch, 1, 1))
        for b in range(batch):
            x[b, :, 2] = d.h_min + SRB_HEIGHTS[b % 3]
        X.append(x); U.append(np.tile(p["Ubar"][None], (batch, 1, 1)))
    x0[:, 2] = X[0][:, 0, 2]
    return _per_problem(phases, X, U), x0


def step_case(name, batch=None):
    kw = {} if batch is None else dict(batch=batch)
    return dict(wb_edges=wb_edges, wb_grf_edges=wb_grf_edges, hkd_edges=hkd_edges, srb_edges=srb_edges)[name](**kw)


def step_option(name):
    return P.hkd_ddp_setting() if name.startswith("hkd") else pkg.mhpc_ddp_setting()


# ------------------------------------------------------------------------------------------------------------- update cases
# (delta, delta_min, eps) per group.  Under update_relax = 0.5: torque 0.5 -> 0.25 -> 0.125 -> 0.1 (clamped: 0.0625 < 0.1), joint speed 0.25 -> 0.125 ->
# 0.0625 (its floor, reached exactly), joint 0.125 -> 0.0625 -> 0.04 (clamped), height 0.03125 -> 0.015625 -> 0.01 (clamped), pyramid 1 -> 0.5 -> 0.3 (clamped).
WB_UPDATE_REB = dict(torque=(0.5, 0.1, 0.1), jointspeed=(0.25, 0.0625, 0.2), joint=(0.125, 0.04, 0.05), minheight=(0.03125, 0.01, 0.15), grf=(1.0, 0.3, 0.3))
HKD_UPDATE_REB = (0.5, 0.1, 0.0009765625)
HKD_UPDATE_R = 10.0
SRB_UPDATE_REB = (0.03125, 0.01, 0.1)
SIGMA_MAX = dict(wb_updates=60.0, hkd_updates=250.0)      # 10 -> 50 -> 60 and 20 -> 100 -> 250: an uncapped product, then the cap


# wb_updates one knot later: the first phase loses its first knot, the last one gains a knot, a phase new to the window follows
WB_SHIFTED = dict(schedule=((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (1, 1, 1, 1)), horizons=(1, 3, 3, 1), last_next=(1, 1, 1, 1))
WB_SHIFT_SRC, WB_SHIFT_BY = (0, 1, 2, -1), (1, 0, 0, 0)


def update_case(name, window=None):
    """(phases, x0, option maker): option(max_AL_iter) is the case's setting with live updates."""
    if name == "wb_updates":
        phases, x0 = wb_edges(batch=6, reb=WB_UPDATE_REB, window=window)
        for p in phases:
            d = p["desc"]; d.torque_limit = 2.0; d.al_td = Al(10.0, 0.0, SIGMA_MAX[name])
        base = pkg.mhpc_ddp_setting
    elif name == "hkd_updates":
        # The pyramid constrains the controls themselves, so a solve walks out of a violation unless the tracking cost holds it there: the force
        # REFERENCE of every contact leg violates one row (in turn over knots and legs), the forces are tracked with weight r = 10 and the barrier
        # starts weak (eps 2^-10): curvature eps / delta^2 = 0.004 against r dt = 0.1, until eps has grown and delta has shrunk.
        phases, x0 = hkd_edges(reb=HKD_UPDATE_REB)
        seen = [0] * 4
        for p in phases:
            d = p["desc"]; d.al_td = Al(20.0, 0.0, SIGMA_MAX[name])
            for i in range(12):
                d.r[i] = HKD_UPDATE_R
            for k in range(d.horizon + 1):
                for l in range(4):
                    if d.contact[l]:
                        p["bufs"]["ur"][k, 3 * l:3 * l + 3] = hkd_edge_force(5 + (3 * seen[l] + l) % 5, d.mu)
                        seen[l] += 1
        base = P.hkd_ddp_setting
    elif name == "srb_updates":
        phases, x0 = srb_edges(reb=SRB_UPDATE_REB)
        base = pkg.mhpc_ddp_setting
    else:
        raise KeyError(name)
    return phases, x0, (lambda n_al: base(update_ReB=UPDATE_REB, update_relax=UPDATE_RELAX, max_AL_iter=n_al, max_DDP_iter=2))


def make(lib, phases, x0, **kw):
    s = pkg.Solver(lib, phases, batch=x0.shape[0], **kw)
    for i, p in enumerate(phases):
        n, m, _ = s.dims[i]
        assert p["Xbar"].shape == (s.batch, s.horizons[i] + 1, n) and p["Ubar"].shape == (s.batch, s.horizons[i], m), (i, p["Xbar"].shape, p["Ubar"].shape)
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    return s


def params(s):
    """{field: [array per phase]} of the four parameter fields."""
    return {f: [s.field(i, f) for i in range(len(s.phases))] for f in PARAM_FIELDS}


def eps_exponent(eps, eps0):
    """How many times an entry was multiplied by update_ReB."""
    return np.rint(np.log(eps / eps0) / np.log(UPDATE_REB)).astype(int)


def initial_params(phases, batch):
    """What a fresh handle holds: per phase (eps0, delta0, floor) [h, ng] from the groups' Reb."""
    out = []
    for p in phases:
        d = p["desc"]; lay = layout(d)
        reb = [group_params(d, g) for _, _, g in lay]
        row = lambda a: np.tile(np.array([getattr(r, a) for r in reb], dtype=np.float64), (batch, d.horizon, 1))
        out.append((row("eps"), row("delta"), row("delta_min")))
    return out


def compare_params(sa, sb, tag, exact=True, surviving=None):
    """REB_EPS, REB_DELTA and AL_SIGMA of two handles bit for bit (exact) or to 1e-12 relative, AL_LAMBDA to 1e-8 x max(1, scale).  surviving: per phase
    a knot slice to compare the barrier parameters on (None: all)."""
    pa, pb = params(sa), params(sb)
    for f in PARAM_FIELDS:
        for i, (a, b) in enumerate(zip(pa[f], pb[f])):
            assert a.shape == b.shape, (tag, f, i, a.shape, b.shape)
            if f.startswith("REB") and surviving is not None:
                a, b = a[:, surviving[i]], b[:, surviving[i]]
            if a.size == 0:
                continue
            if f == "AL_LAMBDA":
                sc = max(1.0, float(np.abs(a).max()))
                assert np.abs(a - b).max() <= 1e-8 * sc, (tag, f, i, float(np.abs(a - b).max()), sc)
            elif exact:
                assert np.array_equal(a, b), (tag, f, i, float(np.abs(a - b).max()), int((a != b).sum()))
            else:
                assert np.allclose(a, b, rtol=1e-12, atol=0.0), (tag, f, i, float(np.abs(a / b - 1).max()))


def worst_ratio(report):
    """Largest error / tolerance of a run_steps or compare_solve report per field group (pattern_common.worst_ratio)."""
    import pattern_common as pt
    return {k: float(f"{v:.3g}") for k, v in pt.worst_ratio(report).items()}


# ------------------------------------------------------------------------------------------------------------- window shift
def shift_window(s):
    """hsddp_reconfigure of a handle holding wb_updates to the window one knot later, the way builder.shift_solver_in_place maps phases
    (src_phase / shift; -1 for a phase new to the window, which then gets its nominal trajectory).  Returns the new phases."""
    phases, _, _ = update_case("wb_updates", window=WB_SHIFTED)
    s.reconfigure(phases, list(WB_SHIFT_SRC), list(WB_SHIFT_BY))
    for i, src in enumerate(WB_SHIFT_SRC):
        if src < 0:
            s.set_nominal(i, phases[i]["Xbar"], phases[i]["Ubar"])
    return phases


def expected_after_shift(before, new_phases, batch):
    """The parameter fields a shift must leave, from those before it (params()): a surviving knot keeps its barrier parameters, a knot pushed
    behind a surviving phase copies the last knot's (PathConstraintBase::push_back), the terminal parameters stay with their phase, and a phase
    new to the window carries the initial values of its descriptor."""
    init = initial_params(new_phases, batch)
    out = {f: [] for f in PARAM_FIELDS}
    for i, (src, by) in enumerate(zip(WB_SHIFT_SRC, WB_SHIFT_BY)):
        d = new_phases[i]["desc"]
        nt = sum(1 for l in range(4) if d.contact[l] == 0 and d.next_contact[l] == 1) if d.c_touchdown else 0
        if src < 0:
            out["REB_EPS"].append(init[i][0]); out["REB_DELTA"].append(init[i][1])
            out["AL_SIGMA"].append(np.full((batch, 1, nt), d.al_td.sigma)); out["AL_LAMBDA"].append(np.full((batch, 1, nt), d.al_td.lambda_))
            continue
        hs = before["REB_EPS"][src].shape[1]
        ks = np.minimum(np.arange(d.horizon) + by, hs - 1)
        out["REB_EPS"].append(before["REB_EPS"][src][:, ks]); out["REB_DELTA"].append(before["REB_DELTA"][src][:, ks])
        out["AL_SIGMA"].append(before["AL_SIGMA"][src]); out["AL_LAMBDA"].append(before["AL_LAMBDA"][src])
    return out
