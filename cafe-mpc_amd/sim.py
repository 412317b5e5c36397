"""Closed-loop rollouts of a solved whole-body policy from perturbed initial states (include/hsddp_sim.h; libhsddp_hip.so only).

    x0 = problems.perturbed_states(solver.field(0, "XBAR")[:, 0], 16, 0.02, 0.2, seed=1)      # [B, 16, 36]
    res = solver.simulate(x0, n_steps=50)              # one-off: creates, runs, reads back, destroys
    res["rows"]["dev_q"], res["rows"]["first_bad"], res["x_final"]

    sim = Simulation(solver, n_samples=16, n_steps=50)  # kept across ticks: run() makes no device allocation
    sim.run(x0); rows, x_final = sim.rows()

    d = Disturbance(seed=7, sigma_u=0.2, sigma_q=1e-3, sigma_v=1e-2, u_max=17.0, fall_height=0.16)      # include/hsddp_mc.h
    res = solver.simulate(x0, n_steps=50, dist=d, kick=kick)      # kick [B, 16, 36] at d.kick_step; res["extra"]["first_fall"], ["n_sat"]

    res = solver.simulate(x0, n_steps=50, keep_traj=True, grf=(0.6, 0.0))      # include/hsddp_grf.h: res["grf"]["min_fz"], ["min_cone"], ["n_slip"], res["Y"]

    res = solver.simulate(x0, n_steps=50, substeps=4)      # include/hsddp_substep.h: four Euler steps of dt / 4 per control knot, torque held

    res = solver.simulate(x0, n_steps=50, contact=(0.0, 0.0))      # include/hsddp_contact.h: the ground only pushes; res["contact"]["n_release"], ["n_land"]

    ter = Terrain(H=heights, x0=-1.0, y0=-1.0, cx=0.05, cy=0.05, early=True, w_td=0.05, map_of=maps)      # include/hsddp_terrain.h: H [n_maps, ny, nx]
    res = solver.simulate(x0, n_steps=50, contact=(0.0, 0.0), terrain=ter)      # res["terrain"]["n_early"], ["max_pen"]

    pl = Plant(np.stack([Plant.nominal().rows[0], with_trunk(Plant.nominal().rows[0], *payload_trunk(1.0, (0.05, 0.0, 0.04)))]), plant_of=idx)
    res = solver.simulate(x0, n_steps=50, substeps=2, plant=pl)      # include/hsddp_plant.h: a plant row per sample, idx int [batch, R]

Nothing here computes anything: the rollout is the k_sim_quad / k_sim_quad_mc kernel (csrc/wb_sim.hpp).  mc_normals states the generator of the
disturbed runs in numpy, grf_rows the contact-force records and grf_rows_sub those of a sub-stepped run, terrain_height the height lookup of a terrain: the definitions the kernel mirrors."""
import ctypes as C
import dataclasses

import numpy as np

from . import _abi
from .problems import SplitMix64


@dataclasses.dataclass
class Disturbance:
    """hsddp_mc_dist_t: the switches of a disturbed run.  A sigma of 0, u_max <= 0, fall_height <= 0 switch their term off."""
    seed: int = 0
    sigma_u: float = 0.0
    sigma_q: float = 0.0
    sigma_v: float = 0.0
    u_max: float = 0.0
    fall_height: float = 0.0
    kick_step: int = 0
    first_problem: int = 0

    def to_c(self):
        return _abi.McDist(self.seed & ((1 << 64) - 1), self.sigma_u, self.sigma_q, self.sigma_v, self.u_max, self.fall_height, self.kick_step, self.first_problem)


@dataclasses.dataclass
class Terrain:
    """hsddp_terrain_t with its grid (include/hsddp_terrain.h): H [n_maps, ny, nx] heights above z_ground (a [ny, nx] array is one map), origin
    (x0, y0), cell size (cx, cy); early: swing feet land when they reach the ground, moving down faster than w_td; map_of: None (map 0 for every
    sample) or int [batch, n_samples]."""
    H: np.ndarray
    x0: float = 0.0
    y0: float = 0.0
    cx: float = 1.0
    cy: float = 1.0
    early: bool = False
    w_td: float = 0.0
    map_of: np.ndarray = None

    def grid(self):
        H = np.ascontiguousarray(self.H, dtype=np.float64)
        return H[None] if H.ndim == 2 else H

    def to_c(self):
        H = self.grid()
        if H.ndim != 3:
            raise ValueError(f"Terrain: H has shape {H.shape}")
        return _abi.TerrainParams(H.shape[2], H.shape[1], H.shape[0], 1 if self.early else 0, self.x0, self.y0, self.cx, self.cy, self.w_td)


class Friction:
    """The friction table of include/hsddp_friction.h: mu [n_mu, 2] rows (mu_s, mu_k) with 0 <= mu_k <= mu_s - a pair (mu_s, mu_k) is one row, a number
    mu means (mu, mu) - mu_of int [batch, R] or None (row 0 for every sample), and v_stick (m/s), the speed below which a sliding foot sticks again."""

    def __init__(self, mu, mu_of=None, v_stick=0.01):
        self.mu, self.mu_of, self.v_stick = mu, mu_of, float(v_stick)

    def table(self):
        m = np.asarray(self.mu, dtype=np.float64)
        if m.ndim == 0:
            m = np.array([[float(m), float(m)]])
        if m.ndim == 1:
            m = m[None]
        if m.ndim != 2 or m.shape[1] != 2:
            raise ValueError(f"Friction: mu has shape {m.shape}")
        return np.ascontiguousarray(m)


def terrain_height(terrain, p_xy, m=0):
    """Height of map m of `terrain` above z_ground at the points p_xy [..., 2]: the definition of the lookup.  ix = clamp(floor((p_x - x0) / cx), 0,
    nx - 1), iy likewise, H[m, iy, ix]: outside the grid the edge cell holds, and a NaN coordinate reads cell 0 (fmax / fmin drop a NaN).  m: an int
    or an int array broadcastable to p_xy's leading shape."""
    H = terrain.grid()
    p = np.asarray(p_xy, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ix = np.fmin(np.fmax(np.floor((p[..., 0] - terrain.x0) / terrain.cx), 0.0), H.shape[2] - 1.0).astype(np.int64)
        iy = np.fmin(np.fmax(np.floor((p[..., 1] - terrain.y0) / terrain.cy), 0.0), H.shape[1] - 1.0).astype(np.int64)
    return H[np.asarray(m, dtype=np.int64), iy, ix]


@dataclasses.dataclass
class Plant:
    """The plant table of include/hsddp_plant.h: rows [n_plants, 46] (a [46] array is one row) and plant_of, None (row 0 for every sample) or int
    [batch, n_samples].  A row: trunk mass | trunk CoM | trunk inertia about its CoM (xx, xy, xz, yy, yz, zz) | link_scale 12 | tau_gain 12 | damping 12,
    joints leg-major (_abi.PLANT_SLICES)."""
    rows: np.ndarray
    plant_of: np.ndarray = None

    def table(self):
        P = np.ascontiguousarray(self.rows, dtype=np.float64)
        P = P[None] if P.ndim == 1 else P
        if P.ndim != 2 or P.shape[1] != _abi.PLANT_ROW:
            raise ValueError(f"Plant: rows have shape {P.shape}")
        return P

    @staticmethod
    def nominal(n=1):
        """n copies of the row the planner believes in."""
        return Plant(np.tile(np.array(_abi.PLANT_NOMINAL), (int(n), 1)))


def payload_trunk(mass, pos, inertia=None):
    """(mass, CoM [3], inertia about the CoM [6: xx, xy, xz, yy, yz, zz]) of the nominal trunk with a payload of `mass` at `pos` (trunk axes) whose
    own inertia about its centre is `inertia` (same six entries; None: a point mass): the parallel-axis composition, which is the definition."""
    nom = np.array(_abi.PLANT_NOMINAL)
    m0, c0 = nom[0], nom[1:4]
    sym = lambda v: np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]], dtype=np.float64)
    about = lambda m, d: m * (float(d @ d) * np.eye(3) - np.outer(d, d))      # a point mass m at d, about the origin
    p = np.asarray(pos, dtype=np.float64)
    m = m0 + float(mass)
    c = (m0 * c0 + float(mass) * p) / m
    Ic = sym(nom[4:10]) + about(m0, c0 - c) + (sym(np.asarray(inertia, dtype=np.float64)) if inertia is not None else 0.0) + about(float(mass), p - c)
    return m, c, np.array([Ic[0, 0], Ic[0, 1], Ic[0, 2], Ic[1, 1], Ic[1, 2], Ic[2, 2]])


def with_trunk(row, mass, com, inertia):
    """A copy of the plant row with the trunk's ten entries replaced (what payload_trunk returns)."""
    out = np.array(row, dtype=np.float64)
    out[0] = mass; out[1:4] = com; out[4:10] = inertia
    return out


def _with_joints(row, name, v):
    out = np.array(row, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size not in (1, 3, 12):
        raise ValueError(f"{name}: {v.size} values, not 1, 3 or 12")
    out[_abi.PLANT_SLICES[name]] = np.tile(v, 12 // v.size)
    return out


def with_link_scale(row, scale):
    """A copy of the row with link_scale set: a scalar, three values (abad, hip, knee of every leg) or twelve (leg-major)."""
    return _with_joints(row, "link_scale", scale)


def with_gain(row, gain):
    """A copy of the row with tau_gain set (scalar, three or twelve values)."""
    return _with_joints(row, "tau_gain", gain)


def with_damping(row, b):
    """A copy of the row with the viscous friction set, N m s / rad (scalar, three or twelve values).  The friction is explicit: see the header."""
    return _with_joints(row, "damping", b)


def mc_normals(seed, problem, r, s):
    """The 48 standard normal numbers of (global problem, sample r, step s) of a disturbed run: coordinate c = 0..11 is added (times sigma_u) to
    the torque of joint c, c = 12..47 (times sigma_q / sigma_v) to state coordinate c - 12 of the estimate.  Coordinate c is Box-Muller on draws
    n0 + 1 and n0 + 2 of SplitMix64(seed), n0 = 2 (((problem 65536 + r) 65536 + s) 48 + c): a function of its arguments alone."""
    if not (problem >= 0 and 0 <= r < 65536 and 0 <= s <= 65536):
        raise ValueError(f"mc_normals: problem {problem}, sample {r}, step {s}")
    rng = SplitMix64(seed)
    rng.skip(2 * 48 * ((problem * 65536 + r) * 65536 + s))
    u = np.array([rng.next() for _ in range(96)])
    return np.sqrt(-2.0 * np.log(1.0 - u[0::2])) * np.cos(2.0 * np.pi * u[1::2])      # 1 - u is in (0, 1]


def grf_rows(Y, contact, mu, fz_min, first_bad=None):
    """The contact-force records of include/hsddp_grf.h from the forces themselves.  Y: [..., n, 12] world-frame contact forces per step (foot l at
    3 l .. 3 l + 2); contact: [n, 4], foot l is a stance foot of step s iff contact[s, l] > 0; first_bad: None, or an int array of Y's leading shape
    - where it is >= 0 only the steps s <= first_bad count (the sample was alive when they began).  Over the stance (foot, step) pairs that count:
    cone = mu fz - max(|fx|, |fy|), a pair violates iff fz < fz_min or cone < 0.  Returns a structured array (GRF_ROW_DTYPE) of Y's leading shape:
    min_fz, min_cone (+inf without a stance pair), max_fz (-inf), first_slip (-1 without a violation), n_slip."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[-2]
    lead = Y.shape[:-2]
    F = Y.reshape(lead + (n, 4, 3))
    st = np.broadcast_to(np.asarray(contact).reshape(n, 4) > 0, lead + (n, 4))
    if first_bad is not None:
        fb = np.asarray(first_bad).reshape(lead + (1, 1))
        st = st & ((fb < 0) | (np.arange(n).reshape(n, 1) <= fb))
    fz = F[..., 2]
    cone = mu * fz - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    viol = st & ((fz < fz_min) | (cone < 0.0))
    out = np.zeros(lead, dtype=_abi.GRF_ROW_DTYPE)
    out["min_fz"] = np.where(st, fz, np.inf).min(axis=(-2, -1), initial=np.inf)
    out["min_cone"] = np.where(st, cone, np.inf).min(axis=(-2, -1), initial=np.inf)
    out["max_fz"] = np.where(st, fz, -np.inf).max(axis=(-2, -1), initial=-np.inf)
    step = viol.any(axis=-1)
    out["first_slip"] = np.where(step.any(axis=-1), step.argmax(axis=-1), -1) if n else -1
    out["n_slip"] = viol.sum(axis=(-2, -1))
    return out


def grf_rows_sub(Y, contact, mu, fz_min, counted=None):
    """The contact-force records of a sub-stepped run (include/hsddp_substep.h) from the forces of every substep.  Y: [..., n, S, 12], the force of
    substep j of control step s; contact: [n, 4] as for grf_rows (a foot stands through all substeps of a step); counted: None, or a boolean array
    [..., n, S] - substep (s, j) counts iff the sample was alive when it began.  min_fz, min_cone and max_fz run over the stance (foot, substep)
    pairs that count; first_slip is the CONTROL step of the first violating substep; n_slip counts violating (foot, substep) pairs.  This is
    grf_rows on the n S flattened substeps with the contact rows repeated and first_slip // S."""
    Y = np.asarray(Y, dtype=np.float64)
    n, S = Y.shape[-3], Y.shape[-2]
    lead = Y.shape[:-3]
    F = Y.reshape(lead + (n, S, 4, 3))
    st = np.broadcast_to((np.asarray(contact).reshape(n, 1, 4) > 0), lead + (n, S, 4))
    if counted is not None:
        st = st & np.asarray(counted, dtype=bool).reshape(lead + (n, S, 1))
    fz = F[..., 2]
    cone = mu * fz - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    viol = st & ((fz < fz_min) | (cone < 0.0))
    out = np.zeros(lead, dtype=_abi.GRF_ROW_DTYPE)
    out["min_fz"] = np.where(st, fz, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["min_cone"] = np.where(st, cone, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["max_fz"] = np.where(st, fz, -np.inf).max(axis=(-3, -2, -1), initial=-np.inf)
    step = viol.any(axis=(-2, -1))
    out["first_slip"] = np.where(step.any(axis=-1), step.argmax(axis=-1), -1) if n else -1
    out["n_slip"] = viol.sum(axis=(-3, -2, -1))
    return out


class Simulation:
    """One hsddp_sim_t on a Solver's handle.  Stale after Solver.reconfigure (run raises; create a new one).  Close it before the solver."""

    def __init__(self, solver, n_samples, n_steps, keep_traj=False):
        self.lib = _abi.bind_sim(solver.lib)      # raises on a library without include/hsddp_sim.h (the CPU checker)
        self.disturbed = False
        self.grf_on = False
        self.contact_on = False
        self.terrain_on = False
        self.plant_on = False
        self.friction_on = False
        self.solver, self.R, self.n_steps, self.keep_traj = solver, int(n_samples), int(n_steps), bool(keep_traj)
        self.s = C.c_void_p()
        rc = self.lib.hsddp_sim_create(solver.h, self.R, self.n_steps, 1 if keep_traj else 0, C.byref(self.s))
        if rc != 0:
            self.s = C.c_void_p()
            raise RuntimeError(f"hsddp_sim_create failed rc={rc}")

    def close(self):
        if self.s:
            self.lib.hsddp_sim_destroy(self.s)
            self.s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _source(self, name, x):
        """(address, on the device, what keeps it alive) of a [B, R, 36] float64 numpy array or contiguous torch tensor on the handle's device."""
        shape = (self.solver.batch, self.R, 36)
        if type(x).__module__.startswith("torch"):
            import torch
            if x.dtype != torch.float64 or not x.is_contiguous() or x.device.type != "cuda" or tuple(x.shape) != shape:
                raise ValueError(f"{name}: need a contiguous float64 tensor of shape {shape} on the handle's device, got {x.dtype} {tuple(x.shape)} on {x.device}")
            torch.cuda.current_stream(x.device).synchronize()      # the kernel runs on the handle's stream
            return x.data_ptr(), 1, x
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != shape:
            raise ValueError(f"{name}: shape {x.shape}, need {shape}")
        return x.ctypes.data, 0, x

    def run(self, x0, dist=None, kick=None):
        """x0: [B, R, 36] float64, a numpy array (copied) or a contiguous torch tensor on the handle's device (read in place).
        dist (Disturbance) and / or kick ([B, R, 36], as x0; added to the state at step dist.kick_step): a disturbed run (include/hsddp_mc.h)."""
        p, dev, keep = self._source("x0", x0)
        if dist is None and kick is None:
            rc = self.lib.hsddp_sim_run(self.s, p, dev)
            if rc != 0:
                raise RuntimeError(f"hsddp_sim_run failed rc={rc}")
            self.disturbed = False
            return
        _abi.bind_mc(self.lib)
        d = (dist if dist is not None else Disturbance()).to_c()
        kp, kdev, kkeep = self._source("kick", kick) if kick is not None else (None, 0, None)
        rc = self.lib.hsddp_mc_run(self.s, p, dev, C.byref(d), kp, kdev)
        if rc != 0:
            raise RuntimeError(f"hsddp_mc_run failed rc={rc}")
        self.disturbed = True

    def extra(self, b0=0, nb=None):
        """Structured array [nb, R] of hsddp_mc_extra_t (first_fall, n_sat) of the last run, which has to be a disturbed one."""
        nb = self.solver.batch - b0 if nb is None else nb
        out = np.zeros((max(nb, 0), self.R), dtype=_abi.MC_EXTRA_DTYPE)
        rc = _abi.bind_mc(self.lib).hsddp_mc_get_extra(self.s, b0, nb, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_mc_get_extra failed rc={rc}")
        return out

    def set_grf(self, mu, fz_min=0.0):
        """Contact-force records (include/hsddp_grf.h) for every later run: mu > 0 switches them on with these thresholds, mu == 0 off."""
        rc = _abi.bind_grf(self.lib).hsddp_grf_set(self.s, float(mu), float(fz_min))
        if rc != 0:
            raise RuntimeError(f"hsddp_grf_set failed rc={rc}")
        self.grf_on = mu > 0

    def set_substeps(self, substeps):
        """Sub-stepped integration (include/hsddp_substep.h) for every later run: S forward-Euler steps of dt / S per control knot under the
        knot's torque, 1 <= S <= 64; 1 is the plain walk."""
        rc = _abi.bind_substep(self.lib).hsddp_substep_set(self.s, int(substeps))
        if rc != 0:
            raise RuntimeError(f"hsddp_substep_set failed rc={rc}")

    def set_contact(self, fz_rel=0.0, z_ground=0.0):
        """Unilateral ground contact (include/hsddp_contact.h) for every later run: a stance foot whose normal force falls below fz_rel is
        released and lands again on the flat ground at world height z_ground."""
        rc = _abi.bind_contact(self.lib).hsddp_contact_set(self.s, 1, float(fz_rel), float(z_ground))
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_set failed rc={rc}")
        self.contact_on = True

    def clear_contact(self):
        """Later runs glue the scheduled stance feet to the ground again (the kernels without the rule)."""
        rc = _abi.bind_contact(self.lib).hsddp_contact_set(self.s, 0, 0.0, 0.0)
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_set failed rc={rc}")
        self.contact_on = False

    @property
    def contact(self):
        """(on, fz_rel, z_ground) as later runs use them (hsddp_contact_get_params)."""
        on = C.c_int(); f = C.c_double(); z = C.c_double()
        rc = _abi.bind_contact(self.lib).hsddp_contact_get_params(self.s, C.byref(on), C.byref(f), C.byref(z))
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_get_params failed rc={rc}")
        return bool(on.value), f.value, z.value

    def contact_rows(self, b0=0, nb=None):
        """Structured array [nb, R] of hsddp_contact_row_t of the last run, which has to be one with the rule on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), self.R), dtype=_abi.CONTACT_ROW_DTYPE)
        rc = _abi.bind_contact(self.lib).hsddp_contact_get(self.s, b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_get failed rc={rc}")
        return rows

    def set_terrain(self, terrain):
        """Terrain height maps and early swing-foot touchdown (include/hsddp_terrain.h) for every later run with the contact rule on; `terrain`: a
        Terrain.  The grid and the map table are copied."""
        H = terrain.grid()
        mo = None if terrain.map_of is None else np.ascontiguousarray(terrain.map_of, dtype=np.int32)
        if mo is not None and mo.shape != (self.solver.batch, self.R):
            raise ValueError(f"Terrain.map_of has shape {mo.shape}, not {(self.solver.batch, self.R)}")
        t = terrain.to_c()
        rc = _abi.bind_terrain(self.lib).hsddp_terrain_set(self.s, 1, C.byref(t), H.ctypes.data, None if mo is None else mo.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_set failed rc={rc}")
        self.terrain_on = True

    def clear_terrain(self):
        """Later runs stand on the plane z_ground again and test scheduled stance feet only (the kernels without the terrain)."""
        rc = _abi.bind_terrain(self.lib).hsddp_terrain_set(self.s, 0, None, None, None)
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_set failed rc={rc}")
        self.terrain_on = False

    @property
    def terrain(self):
        """(on, dict of nx, ny, n_maps, early, x0, y0, cx, cy, w_td) as later runs use them (hsddp_terrain_get_params)."""
        on = C.c_int(); t = _abi.TerrainParams()
        rc = _abi.bind_terrain(self.lib).hsddp_terrain_get_params(self.s, C.byref(on), C.byref(t))
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_get_params failed rc={rc}")
        return bool(on.value), {f: getattr(t, f) for f, _ in _abi.TerrainParams._fields_}

    def terrain_rows(self, b0=0, nb=None):
        """Structured array [nb, R] of hsddp_terrain_row_t of the last run, which has to be one with the contact rule and the terrain on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), self.R), dtype=_abi.TERRAIN_ROW_DTYPE)
        rc = _abi.bind_terrain(self.lib).hsddp_terrain_get(self.s, b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_get failed rc={rc}")
        return rows

    def set_friction(self, friction):
        """Coulomb friction (include/hsddp_friction.h) for every later run with the contact rule on; `friction`: a Friction.  The table and the index
        are copied.  A run with friction and a plant both on raises (HSDDP_ENOTSUP)."""
        mu = friction.table()
        mo = None if friction.mu_of is None else np.ascontiguousarray(friction.mu_of, dtype=np.int32)
        if mo is not None and mo.shape != (self.solver.batch, self.R):
            raise ValueError(f"Friction.mu_of has shape {mo.shape}, not {(self.solver.batch, self.R)}")
        f = _abi.FrictionParams(friction.v_stick, mu.shape[0], 0)
        rc = _abi.bind_friction(self.lib).hsddp_friction_set(self.s, 1, C.byref(f), mu.ctypes.data, None if mo is None else mo.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_set failed rc={rc}")
        self.friction_on = True

    def clear_friction(self):
        """Later runs hold every attached foot with three rows again (the kernels without friction)."""
        rc = _abi.bind_friction(self.lib).hsddp_friction_set(self.s, 0, None, None, None)
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_set failed rc={rc}")
        self.friction_on = False

    @property
    def friction(self):
        """(on, dict of v_stick, n_mu) as later runs use them (hsddp_friction_get_params)."""
        on = C.c_int(); f = _abi.FrictionParams()
        rc = _abi.bind_friction(self.lib).hsddp_friction_get_params(self.s, C.byref(on), C.byref(f))
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_get_params failed rc={rc}")
        return bool(on.value), dict(v_stick=f.v_stick, n_mu=f.n_mu)

    def friction_rows(self, b0=0, nb=None):
        """Structured array [nb, R] of hsddp_friction_row_t of the last run, which has to be one with the contact rule and friction on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), self.R), dtype=_abi.FRICTION_ROW_DTYPE)
        rc = _abi.bind_friction(self.lib).hsddp_friction_get(self.s, b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_get failed rc={rc}")
        return rows

    def set_plant(self, plant):
        """A plant row per sample for every later run (include/hsddp_plant.h); `plant`: a Plant.  The table and the index are copied."""
        P = plant.table()
        po = None if plant.plant_of is None else np.ascontiguousarray(plant.plant_of, dtype=np.int32)
        if po is not None and po.shape != (self.solver.batch, self.R):
            raise ValueError(f"Plant.plant_of has shape {po.shape}, not {(self.solver.batch, self.R)}")
        rc = _abi.bind_plant(self.lib).hsddp_plant_set(self.s, 1, P.shape[0], P.ctypes.data, None if po is None else po.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_plant_set failed rc={rc}")
        self.plant_on = True

    def clear_plant(self):
        """Later runs simulate the planner's robot again (the kernels without the plant)."""
        rc = _abi.bind_plant(self.lib).hsddp_plant_set(self.s, 0, 0, None, None)
        if rc != 0:
            raise RuntimeError(f"hsddp_plant_set failed rc={rc}")
        self.plant_on = False

    @property
    def plant(self):
        """(on, rows [n_plants, 46]) as later runs use them (hsddp_plant_get_params, hsddp_plant_get_table); no rows on a fresh object."""
        lib = _abi.bind_plant(self.lib)
        on = C.c_int(); n = C.c_int()
        rc = lib.hsddp_plant_get_params(self.s, C.byref(on), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"hsddp_plant_get_params failed rc={rc}")
        P = np.zeros((n.value, _abi.PLANT_ROW))
        if n.value > 0:
            rc = lib.hsddp_plant_get_table(self.s, 0, n.value, P.ctypes.data)
            if rc != 0:
                raise RuntimeError(f"hsddp_plant_get_table failed rc={rc}")
        return bool(on.value), P

    @property
    def substeps(self):
        """What later runs use, as the library reports it (hsddp_substep_get)."""
        v = C.c_int()
        rc = _abi.bind_substep(self.lib).hsddp_substep_get(self.s, C.byref(v))
        if rc != 0:
            raise RuntimeError(f"hsddp_substep_get failed rc={rc}")
        return v.value

    def grf(self, b0=0, nb=None):
        """Structured array [nb, R] of hsddp_grf_row_t of the last run, which has to be one with the records on; with keep_traj the pair
        (rows, Y [nb, R, n_steps, 12])."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), self.R), dtype=_abi.GRF_ROW_DTYPE)
        Y = np.zeros((max(nb, 0), self.R, self.n_steps, 12)) if self.keep_traj else None
        rc = _abi.bind_grf(self.lib).hsddp_grf_get(self.s, b0, nb, rows.ctypes.data, Y.ctypes.data if Y is not None else None)
        if rc != 0:
            raise RuntimeError(f"hsddp_grf_get failed rc={rc}")
        return (rows, Y) if self.keep_traj else rows

    def rows(self, b0=0, nb=None):
        """(rows [nb, R] as a structured array of hsddp_sim_row_t, x_final [nb, R, 36]) of the last run."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0), self.R), dtype=_abi.SIM_ROW_DTYPE); xf = np.zeros((max(nb, 0), self.R, 36))
        rc = self.lib.hsddp_sim_get_rows(self.s, b0, nb, rows.ctypes.data, xf.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_sim_get_rows failed rc={rc}")
        return rows, xf

    def traj(self, b0=0, nb=None):
        """(X [nb, R, n_steps + 1, 36], U [nb, R, n_steps, 12]) of the last run; needs keep_traj."""
        nb = self.solver.batch - b0 if nb is None else nb
        X = np.zeros((max(nb, 0), self.R, self.n_steps + 1, 36)); U = np.zeros((max(nb, 0), self.R, self.n_steps, 12))
        rc = self.lib.hsddp_sim_get_traj(self.s, b0, nb, X.ctypes.data, U.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_sim_get_traj failed rc={rc}")
        return X, U

    def device_final(self):
        """Device address of the final states [B, R, 36] of the last run (valid while the object lives)."""
        return int(self.lib.hsddp_sim_device_final(self.s) or 0)

    def kernel_time_ms(self):
        ms = C.c_float()
        rc = self.lib.hsddp_sim_get_kernel_time_ms(self.s, C.byref(ms))
        if rc != 0:
            raise RuntimeError(f"hsddp_sim_get_kernel_time_ms failed rc={rc}")
        return float(ms.value)


def simulate(solver, x0, n_steps, keep_traj=False, dist=None, kick=None, grf=None, substeps=1, contact=None, terrain=None, plant=None, friction=None):
    """One-off simulation on `solver`: dict with rows, x_final and, with keep_traj, X and U (see Simulation); a disturbed run (dist / kick given)
    returns extra too; grf = (mu, fz_min) adds the contact-force records grf and, with keep_traj, Y; substeps = S > 1 integrates every control
    knot in S steps (include/hsddp_substep.h); contact = (fz_rel, z_ground) switches unilateral ground contact on (include/hsddp_contact.h) and
    adds the rows contact; terrain = Terrain(...) beside it switches height maps and early touchdown on (include/hsddp_terrain.h) and adds the rows
    terrain; plant = Plant(...) gives every sample a plant row (include/hsddp_plant.h); friction = Friction(...) beside contact lets attached feet slide
    (include/hsddp_friction.h) and adds the rows friction."""
    sim = Simulation(solver, x0.shape[1], n_steps, keep_traj)
    try:
        if substeps != 1:
            sim.set_substeps(substeps)
        if grf is not None:
            sim.set_grf(*grf)
        if contact is not None:
            sim.set_contact(*contact)
        if terrain is not None:
            sim.set_terrain(terrain)
        if plant is not None:
            sim.set_plant(plant)
        if friction is not None:
            sim.set_friction(friction)
        sim.run(x0, dist=dist, kick=kick)
        rows, xf = sim.rows()
        out = dict(rows=rows, x_final=xf)
        if sim.disturbed:
            out["extra"] = sim.extra()
        if keep_traj:
            out["X"], out["U"] = sim.traj()
        if sim.grf_on:
            if keep_traj:
                out["grf"], out["Y"] = sim.grf()
            else:
                out["grf"] = sim.grf()
        if sim.contact_on:
            out["contact"] = sim.contact_rows()
        if sim.contact_on and sim.terrain_on:
            out["terrain"] = sim.terrain_rows()
        if sim.contact_on and sim.friction_on:
            out["friction"] = sim.friction_rows()
        return out
    finally:
        sim.close()
