"""Batched closed-loop MPC episodes (include/hsddp_episode.h; libhsddp_hip.so only): B robots, each running its own MPC against the simulated
whole-body dynamics, with the simulated state handed to the next solve on the device.

    ep = solver.episode(n_exec=2, max_ticks=50, keep_log=True)      # or Episode(solver, 2, 50, True)
    ep.set_grf(0.6)                                                 # optional: contact-force records (include/hsddp_grf.h)
    ep.set_substeps(4)                                              # optional: sub-stepped integration (include/hsddp_substep.h)
    ep.set_contact(0.0, 0.0)                                        # optional: unilateral ground contact (include/hsddp_contact.h)
    ep.set_terrain(sim.Terrain(H=heights, cx=0.05, cy=0.05, early=True, w_td=0.05))      # optional, with it: terrain and early touchdown (include/hsddp_terrain.h)
    ep.set_plant(sim.Plant(rows, plant_of=idx))                     # optional: a plant row per robot, idx int [B] (include/hsddp_plant.h)
    ep.set_latency([0, 1, 2, ...])                                  # optional: policy latency in control steps per robot, int or int [B] (include/hsddp_latency.h)
    ep.reset(x0)                                                    # [B, 36]; also the solver's initial condition
    solver.solve(opt)
    out = run_mhpc(solver, pd, phases, opt_rt, 50, dist=Disturbance(seed=7, sigma_u=0.2, fall_height=0.12), episode=ep)
    rows, x_now = ep.rows(); X, U, Y = ep.log(); tick, n_alive, n_impacts = ep.status()

Nothing here computes anything on the product path: the walk is the kernel of sim.Simulation, the commit and the pending reset map are
k_episode_commit / k_episode_impact (csrc/episode.hpp), and with latency k_episode_latency composes the policy rows the walk applies.  tick_seed,
fold_rows and compose_policy state the seed schedule, the commit and the composition in numpy: the definitions the library mirrors."""
import ctypes as C
import dataclasses

import numpy as np

from . import _abi
from .sim import Disturbance

_M64 = (1 << 64) - 1


def tick_seed(seed, t):
    """Seed of the noise of tick t: the seed itself for t = 0, else the t-th raw 64-bit output of SplitMix64(seed) (problems.SplitMix64: the state
    after t steps, mixed, before the shift that makes a double of it)."""
    seed &= _M64
    if t == 0:
        return seed
    z = (seed + t * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def empty_rows(n):
    """The rows a reset leaves: nothing seen yet."""
    r = np.zeros(n, dtype=_abi.EPISODE_ROW_DTYPE)
    r["min_height"] = np.inf; r["min_fz"] = np.inf; r["min_cone"] = np.inf; r["max_fz"] = -np.inf; r["first_slip"] = -1; r["end_step"] = -1
    return r


def fold_rows(rows, tick, sim_rows, X, U, q, r, xr, ur, extra=None, grf=None, status=None):
    """The commit of one tick into the episode rows (k_episode_commit), for the problems alive at the start of the tick (end_reason == 0); the
    others are returned unchanged.  rows: [B] EPISODE_ROW_DTYPE before the tick; sim_rows: [B] SIM_ROW_DTYPE of the tick's walk; X [B, n + 1, 36],
    U [B, n, 12]: the tick's trajectory; q [n, 36], r [n, 12]: the weights of the phase each step maps to; xr [B or 1, n, 36], ur [B or 1, n, 12]: the
    reference rows of the steps' knots; extra: [B] MC_EXTRA_DTYPE of a disturbed walk or None; grf: [B] GRF_ROW_DTYPE with the force records on or
    None; status: [B] status of the handle's last solve or None.  Returns the rows after the tick."""
    out = rows.copy()
    n = U.shape[1]
    base = tick * n
    live = rows["end_reason"] == 0
    for f in ("dev_q", "dev_v", "max_torque"):
        out[f] = np.where(live, np.fmax(rows[f], sim_rows[f]), rows[f])
    out["min_height"] = np.where(live, np.fmin(rows["min_height"], sim_rows["min_height"]), rows["min_height"])
    if extra is not None:
        out["n_sat"] = np.where(live, rows["n_sat"] + extra["n_sat"], rows["n_sat"])
    if grf is not None:
        out["min_fz"] = np.where(live, np.fmin(rows["min_fz"], grf["min_fz"]), rows["min_fz"])
        out["min_cone"] = np.where(live, np.fmin(rows["min_cone"], grf["min_cone"]), rows["min_cone"])
        out["max_fz"] = np.where(live, np.fmax(rows["max_fz"], grf["max_fz"]), rows["max_fz"])
        out["first_slip"] = np.where(live & (rows["first_slip"] < 0) & (grf["first_slip"] >= 0), base + grf["first_slip"], rows["first_slip"])
        out["n_slip"] = np.where(live, rows["n_slip"] + grf["n_slip"], rows["n_slip"])
    out["steps"] = np.where(live, rows["steps"] + n, rows["steps"])
    if status is not None:
        out["bad_solves"] = np.where(live & (np.asarray(status) == 1), rows["bad_solves"] + 1, rows["bad_solves"])
    dx = X[:, :n] - xr; du = U - ur
    cost = 0.5 * (q[None] * dx * dx).sum(axis=(1, 2)) + 0.5 * (r[None] * du * du).sum(axis=(1, 2))
    out["track_cost"] = np.where(live, rows["track_cost"] + cost, rows["track_cost"])
    fb = sim_rows["first_bad"]
    ff = extra["first_fall"] if extra is not None else np.full(len(rows), -1)
    fell = (ff >= 0) & ((fb < 0) | (ff <= fb))
    reason = np.where(fell, 2, np.where(fb >= 0, 1, 0))
    step = np.where(fell, ff, fb)
    out["end_reason"] = np.where(live, reason, rows["end_reason"])
    out["end_step"] = np.where(live & (reason != 0), base + step, rows["end_step"])
    return out


def step_weights(phases, smap):
    """q [n, 36], r [n, 12] of the phases the steps of a step map (3 x n: phase, knot, reset) belong to."""
    q = np.array([[phases[p]["desc"].q[i] for i in range(36)] for p in smap[0]])
    r = np.array([[phases[p]["desc"].r[j] for j in range(12)] for p in smap[0]])
    return q, r


def step_refs(solver, smap):
    """xr [B, n, 36], ur [B, n, 12]: the reference rows every problem tracks at the knots of a step map (hsddp_get_references)."""
    refs = {p: solver.get_references(int(p)) for p in set(int(p) for p in smap[0])}
    xr = np.stack([refs[int(p)]["xr"][:, k] for p, k in zip(smap[0], smap[1])], axis=1)
    ur = np.stack([refs[int(p)]["ur"][:, k] for p, k in zip(smap[0], smap[1])], axis=1)
    return xr, ur


def latency_step_map(phases, n_steps):
    """The step map (3 x n_steps: phase, knot, reset map behind the step) over the leading whole-body control knots of a window given as the
    builder's phase dicts: what hsddp_sim_create lays out, and with n_steps = n_exec + D the long map of a tick with latency."""
    out = []
    for i, p in enumerate(phases):
        d = p["desc"]
        if d.model != 0:
            break
        td = any(d.contact[l] == 0 and d.next_contact[l] == 1 for l in range(4))
        for k in range(d.horizon):
            out.append([i, k, 1 if (td and k == d.horizon - 1) else 0])
    if len(out) < n_steps:
        raise ValueError(f"the window leads with {len(out)} whole-body knots, not {n_steps}")
    out = out[:n_steps]
    out[-1][2] = 0
    return np.ascontiguousarray(np.array(out, dtype=np.int32).T)


def policy_rows(solver, smap, fields=None):
    """[B, n, 516]: the policy rows Xbar[k] | Xbar[k+1] | Ubar[k] | K[k] (K column-major 12 x 36, the handle's order) of the (phase, knot) pairs of a
    step map.  fields: {phase: (XBAR, UBAR, K)} as Solver.field returns them - a snapshot taken earlier; None reads the solver now."""
    ph = sorted(set(int(p) for p in smap[0]))
    if fields is None:
        fields = {p: (solver.field(p, "XBAR"), solver.field(p, "UBAR"), solver.field(p, "K")) for p in ph}
    rows = []
    for p, k in zip(smap[0], smap[1]):
        X, U, K = fields[int(p)]
        rows.append(np.concatenate([X[:, k], X[:, k + 1], U[:, k], K[:, k].transpose(0, 2, 1).reshape(K.shape[0], 432)], axis=1))
    return np.ascontiguousarray(np.stack(rows, axis=1))


def compose_policy(prev_rows, cur_rows, delay_of, valid):
    """The effective policy of a tick with latency (k_episode_latency), [B, n_exec, 516].  cur_rows [B, n_exec, 516]: the rows of the handle's
    current policy at steps 0 .. n_exec - 1; prev_rows [B, D, 516] or None: the rows the PREVIOUS tick's policy held at its steps n_exec ..
    n_exec + D - 1, the same physical time; delay_of int [B]; valid: the previous advance left those rows (it ran with latency on, after the last
    reset).  Step s of robot b takes prev_rows[b, s] if valid and s < delay_of[b], else cur_rows[b, s]."""
    out = np.array(cur_rows, dtype=np.float64, copy=True)
    if valid:
        for b, d in enumerate(np.asarray(delay_of).reshape(-1)):
            out[b, :d] = prev_rows[b, :d]
    return out


def split_policy(rows):
    """[B, n, 516] rows -> (Xe [B, n, 2, 36], Ue [B, n, 12], Ke [B, n, 432]), the layout of hsddp_latency_get_policy."""
    return rows[..., :72].reshape(rows.shape[:-1] + (2, 36)), rows[..., 72:84], rows[..., 84:]


class Episode:
    """One hsddp_episode_t on a Solver's handle.  Survives Solver.reconfigure (advance rebinds its step map).  Close it before the solver."""

    def __init__(self, solver, n_exec, max_ticks, keep_log=False):
        self.lib = _abi.bind_episode(solver.lib)      # raises on a library without include/hsddp_episode.h (the CPU checker)
        self.solver, self.n_exec, self.max_ticks, self.keep_log = solver, int(n_exec), int(max_ticks), bool(keep_log)
        self.e = C.c_void_p()
        rc = self.lib.hsddp_episode_create(solver.h, self.n_exec, self.max_ticks, 1 if keep_log else 0, C.byref(self.e))
        if rc != 0:
            self.e = C.c_void_p()
            raise RuntimeError(f"hsddp_episode_create failed rc={rc}")

    def close(self):
        if self.e:
            self.lib.hsddp_episode_destroy(self.e)
            self.e = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _source(self, name, x):
        """(address, on the device, what keeps it alive) of a [B, 36] float64 numpy array or contiguous torch tensor on the handle's device."""
        shape = (self.solver.batch, 36)
        if type(x).__module__.startswith("torch"):
            import torch
            if x.dtype != torch.float64 or not x.is_contiguous() or x.device.type != "cuda" or tuple(x.shape) != shape:
                raise ValueError(f"{name}: need a contiguous float64 tensor of shape {shape} on the handle's device, got {x.dtype} {tuple(x.shape)} on {x.device}")
            torch.cuda.current_stream(x.device).synchronize()      # the copy runs on the handle's stream
            return x.data_ptr(), 1, x
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != shape:
            raise ValueError(f"{name}: shape {x.shape}, need {shape}")
        return x.ctypes.data, 0, x

    def reset(self, x0):
        """x0 [B, 36]: the states of tick 0 and the solver's initial condition; rows and log emptied, tick = 0."""
        p, dev, keep = self._source("x0", x0)
        rc = self.lib.hsddp_episode_reset(self.e, p, dev)
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_reset failed rc={rc}")

    def set_grf(self, mu, fz_min=0.0):
        """Contact-force records (include/hsddp_grf.h) for every later tick: mu > 0 on with these thresholds, mu == 0 off."""
        rc = self.lib.hsddp_grf_set(self.lib.hsddp_episode_sim(self.e), float(mu), float(fz_min))
        if rc != 0:
            raise RuntimeError(f"hsddp_grf_set failed rc={rc}")

    def set_substeps(self, substeps):
        """Sub-stepped integration (include/hsddp_substep.h) for every later tick: S Euler steps of dt / S per control knot, torque held."""
        rc = _abi.bind_substep(self.lib).hsddp_substep_set(self.lib.hsddp_episode_sim(self.e), int(substeps))
        if rc != 0:
            raise RuntimeError(f"hsddp_substep_set failed rc={rc}")

    def set_contact(self, fz_rel=0.0, z_ground=0.0, on=True):
        """Unilateral ground contact (include/hsddp_contact.h) for every later tick; the free feet of a robot are carried from tick to tick and
        cleared by reset.  on = False: the scheduled stance feet are glued to the ground again."""
        rc = _abi.bind_contact(self.lib).hsddp_contact_set(self.lib.hsddp_episode_sim(self.e), 1 if on else 0, float(fz_rel), float(z_ground))
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_set failed rc={rc}")

    def contact_rows(self, b0=0, nb=None):
        """Structured array [nb] of hsddp_contact_row_t of the last tick, which has to be one with the rule on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0),), dtype=_abi.CONTACT_ROW_DTYPE)
        rc = _abi.bind_contact(self.lib).hsddp_contact_get(self.lib.hsddp_episode_sim(self.e), b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_contact_get failed rc={rc}")
        return rows

    def set_terrain(self, terrain, on=True):
        """Terrain height maps and early swing-foot touchdown (include/hsddp_terrain.h) for every later tick with the contact rule on; `terrain`: a
        sim.Terrain whose map_of, if given, is int [batch] or [batch, 1].  The swing feet a robot holds are carried from tick to tick and cleared
        by reset.  on = False: the plane and the scheduled stance feet alone again."""
        lib = _abi.bind_terrain(self.lib)
        if not on:
            rc = lib.hsddp_terrain_set(self.lib.hsddp_episode_sim(self.e), 0, None, None, None)
        else:
            H = terrain.grid()
            mo = None if terrain.map_of is None else np.ascontiguousarray(terrain.map_of, dtype=np.int32).reshape(-1)
            if mo is not None and mo.shape != (self.solver.batch,):
                raise ValueError(f"Terrain.map_of has {mo.size} entries, not {self.solver.batch}")
            t = terrain.to_c()
            rc = lib.hsddp_terrain_set(self.lib.hsddp_episode_sim(self.e), 1, C.byref(t), H.ctypes.data, None if mo is None else mo.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_set failed rc={rc}")

    def plan_terrain(self):
        """Terrain-aware planning (include/hsddp_touchdown.h): the touchdown heights of the solver's current window from the terrain this episode
        simulates on - its grid, z_ground and the map of each robot, as they are on the device.  Call it after the window moved (reconfigure, any
        set_references) and before the solve.  Raises if the episode has no terrain set."""
        rc = _abi.bind_touchdown(self.lib).hsddp_episode_plan_terrain(self.e)
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_plan_terrain failed rc={rc}")

    def plan_friction(self, kappa=1.0):
        """Friction-aware planning (include/hsddp_limits.h): mu of the solver's limits row of robot b <- kappa * mu_s of the friction row this episode
        simulates robot b on, read on the device (0 < kappa <= 1: the planner's margin inside the cone).  The other limits of the rows stay as they
        are, and the rows stay across the ticks' reconfigures: one call after set_friction serves the episode.  Raises if no friction is set."""
        rc = _abi.bind_limits(self.lib).hsddp_episode_plan_friction(self.e, float(kappa))
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_plan_friction failed rc={rc}")

    def set_friction(self, friction, on=True):
        """Coulomb friction (include/hsddp_friction.h) for every later tick with the contact rule on; `friction`: a sim.Friction whose mu_of, if
        given, is int [batch] or [batch, 1].  The sliding feet of a robot and their lagged normal forces are carried from tick to tick and cleared by
        reset.  on = False: every attached foot is held with three rows again.  A tick with friction and a plant both on raises (HSDDP_ENOTSUP)."""
        lib = _abi.bind_friction(self.lib)
        if not on:
            rc = lib.hsddp_friction_set(self.lib.hsddp_episode_sim(self.e), 0, None, None, None)
        else:
            mu = friction.table()
            mo = None if friction.mu_of is None else np.ascontiguousarray(friction.mu_of, dtype=np.int32).reshape(-1)
            if mo is not None and mo.shape != (self.solver.batch,):
                raise ValueError(f"Friction.mu_of has {mo.size} entries, not {self.solver.batch}")
            f = _abi.FrictionParams(friction.v_stick, mu.shape[0], 0)
            rc = lib.hsddp_friction_set(self.lib.hsddp_episode_sim(self.e), 1, C.byref(f), mu.ctypes.data, None if mo is None else mo.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_set failed rc={rc}")

    def friction_rows(self, b0=0, nb=None):
        """Structured array [nb] of hsddp_friction_row_t of the last tick, which has to be one with the contact rule and friction on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0),), dtype=_abi.FRICTION_ROW_DTYPE)
        rc = _abi.bind_friction(self.lib).hsddp_friction_get(self.lib.hsddp_episode_sim(self.e), b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_friction_get failed rc={rc}")
        return rows

    def set_plant(self, plant, on=True):
        """A plant row per robot for every later tick (include/hsddp_plant.h); `plant`: a sim.Plant whose plant_of, if given, is int [batch] or
        [batch, 1].  Each robot keeps its plant for the whole episode: the table survives reconfigure and reset, and the reset map that is pending
        at the end of a tick uses the robot's own inertias.  on = False: the planner's robot again."""
        lib = _abi.bind_plant(self.lib)
        if not on:
            rc = lib.hsddp_plant_set(self.lib.hsddp_episode_sim(self.e), 0, 0, None, None)
        else:
            P = plant.table()
            po = None if plant.plant_of is None else np.ascontiguousarray(plant.plant_of, dtype=np.int32).reshape(-1)
            if po is not None and po.shape != (self.solver.batch,):
                raise ValueError(f"Plant.plant_of has {po.size} entries, not {self.solver.batch}")
            rc = lib.hsddp_plant_set(self.lib.hsddp_episode_sim(self.e), 1, P.shape[0], P.ctypes.data, None if po is None else po.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_plant_set failed rc={rc}")

    def set_latency(self, delay):
        """Per-robot policy latency (include/hsddp_latency.h) for every later tick: delay, an int for all or int [batch], in control steps within
        [0, n_exec].  The first steps of a tick then apply the policy of the previous tick.  The next tick runs fresh."""
        lib = _abi.bind_latency(self.lib)
        if np.ndim(delay) == 0:
            rc = lib.hsddp_latency_set(self.e, 1, None, int(delay))
        else:
            d = np.ascontiguousarray(delay, dtype=np.int32).reshape(-1)
            if d.shape != (self.solver.batch,):
                raise ValueError(f"delay has {d.size} entries, not {self.solver.batch}")
            rc = lib.hsddp_latency_set(self.e, 1, d.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"hsddp_latency_set failed rc={rc}")

    def clear_latency(self):
        """Latency off: later ticks apply the handle's policy from their first step, with the launches of an episode that never had it on."""
        rc = _abi.bind_latency(self.lib).hsddp_latency_set(self.e, 0, None, 0)
        if rc != 0:
            raise RuntimeError(f"hsddp_latency_set failed rc={rc}")

    def latency_rows(self, b0=0, nb=None):
        """Structured array [nb] of hsddp_latency_row_t: delay, and the stale steps executed while alive since the reset."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0),), dtype=_abi.LATENCY_ROW_DTYPE)
        rc = _abi.bind_latency(self.lib).hsddp_latency_get(self.e, b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_latency_get failed rc={rc}")
        return rows

    def applied_policy(self, b0=0, nb=None):
        """(Xe [nb, n_exec, 2, 36], Ue [nb, n_exec, 12], Ke [nb, n_exec, 432]): the effective policy the last tick walked, which has to be one with
        latency on.  Xe[:, s, 1] is the knot behind step s in its phase; Ke is column-major 12 x 36."""
        nb = self.solver.batch - b0 if nb is None else nb
        n = self.n_exec
        Xe = np.zeros((max(nb, 0), n, 2, 36)); Ue = np.zeros((max(nb, 0), n, 12)); Ke = np.zeros((max(nb, 0), n, 432))
        rc = _abi.bind_latency(self.lib).hsddp_latency_get_policy(self.e, b0, nb, Xe.ctypes.data, Ue.ctypes.data, Ke.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_latency_get_policy failed rc={rc}")
        return Xe, Ue, Ke

    def terrain_rows(self, b0=0, nb=None):
        """Structured array [nb] of hsddp_terrain_row_t of the last tick, which has to be one with the contact rule and the terrain on."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros((max(nb, 0),), dtype=_abi.TERRAIN_ROW_DTYPE)
        rc = _abi.bind_terrain(self.lib).hsddp_terrain_get(self.lib.hsddp_episode_sim(self.e), b0, nb, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_terrain_get failed rc={rc}")
        return rows

    @property
    def substeps(self):
        v = C.c_int()
        rc = _abi.bind_substep(self.lib).hsddp_substep_get(self.lib.hsddp_episode_sim(self.e), C.byref(v))
        if rc != 0:
            raise RuntimeError(f"hsddp_substep_get failed rc={rc}")
        return v.value

    def advance(self, dist=None, kick=None):
        """One tick: n_exec steps of the solver's current policy from the episode's states, committed and handed to the solver.  dist
        (sim.Disturbance; its seed is the episode's, the tick's is tick_seed) and / or kick ([B, 36] at step dist.kick_step of the tick)."""
        if dist is None and kick is not None:
            dist = Disturbance()
        d = dist.to_c() if dist is not None else None
        kp, kdev, keep = self._source("kick", kick) if kick is not None else (None, 0, None)
        rc = self.lib.hsddp_episode_advance(self.e, C.byref(d) if d is not None else None, kp, kdev)
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_advance failed rc={rc}")

    def rows(self, b0=0, nb=None):
        """(rows [nb] as a structured array of hsddp_episode_row_t, the current states [nb, 36])."""
        nb = self.solver.batch - b0 if nb is None else nb
        rows = np.zeros(max(nb, 0), dtype=_abi.EPISODE_ROW_DTYPE); x = np.zeros((max(nb, 0), 36))
        rc = self.lib.hsddp_episode_get_rows(self.e, b0, nb, rows.ctypes.data, x.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_get_rows failed rc={rc}")
        return rows, x

    def log(self, b0=0, nb=None):
        """(X [nb, max_ticks n_exec + 1, 36], U, Y [nb, max_ticks n_exec, 12]); needs keep_log.  Entries behind the ticks made so far are zero."""
        nb = self.solver.batch - b0 if nb is None else nb
        n = self.max_ticks * self.n_exec
        X = np.zeros((max(nb, 0), n + 1, 36)); U = np.zeros((max(nb, 0), n, 12)); Y = np.zeros((max(nb, 0), n, 12))
        rc = self.lib.hsddp_episode_get_log(self.e, b0, nb, X.ctypes.data, U.ctypes.data, Y.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_get_log failed rc={rc}")
        return X, U, Y

    def state(self):
        """Device address of the current states [B, 36] (valid while the object lives)."""
        return int(self.lib.hsddp_episode_device_state(self.e) or 0)

    def status(self):
        """(ticks advanced since the last reset, problems still alive, reset maps applied by advance)."""
        t, a, i = C.c_int(), C.c_int(), C.c_int()
        rc = self.lib.hsddp_episode_status(self.e, C.byref(t), C.byref(a), C.byref(i))
        if rc != 0:
            raise RuntimeError(f"hsddp_episode_status failed rc={rc}")
        return t.value, a.value, i.value


def run_mhpc(solver, pd, phases, opt_rt, n_ticks, dist=None, kicks=None, hook=None, episode=None, keep_log=False, delay=None, friction=None, plan_terrain=False, post_hook=None, weight_scales=None, limits=None, plan_friction=None):
    """The receding-horizon loop of MHPCLocomotion::update with the SIMULATED state fed back, for the whole batch.  solver: solved for the window
    `phases` of pd (builder.MHPCProblemData).  Per tick: episode.advance, pd.update(), builder.shift_solver_in_place, hook(tick, phases) - the
    place for solver.set_references - and solver.solve(opt_rt).  kicks: {tick: (kick_step, [B, 36])}.  episode: an Episode already reset; None
    creates one (n_exec = dt_mpc / dt_wb, max_ticks = n_ticks) and resets it to the solver's Xbar[0].  delay: None leaves the episode as it is; an int
    or int [B] is Episode.set_latency before the first tick (include/hsddp_latency.h: the loop moves the window by n_exec knots a tick, as that needs).
    friction: None leaves the episode as it is; a sim.Friction is Episode.set_friction before the first tick (it acts while the contact rule is on).
    plan_terrain: every tick, after the hook and before the solve, episode.plan_terrain() gives the new window the touchdown heights of the episode's
    terrain (include/hsddp_touchdown.h); False plans onto the descriptors' ground_height.  post_hook(tick, phases) is called after the tick's solve.
    weight_scales: None leaves the solver as it is; (sq, sr, sqf) is Solver.set_weight_scales before the first tick (include/hsddp_weights.h) - set once,
    the scales stay across the ticks' reconfigures; the episode's track_cost goes on using the descriptors' weights.
    limits: None leaves the solver as it is; a dict of Solver.set_limits' keyword arguments is that call before the first tick (include/hsddp_limits.h).
    plan_friction: None plans with the limits as they are; a kappa is Episode.plan_friction(kappa) before the first tick, after `friction` and `limits`
    (set once: the rows stay across the ticks' reconfigures).  Returns a dict: episode, phases (the last
    window), n_iters / n_ls_iters / n_reg_iters / cost [n_ticks, B], alive [n_ticks]."""
    from . import builder
    if episode is None:
        episode = Episode(solver, int(round(float(pd.cfg["dt_mpc"]) / pd.dt_wb)), n_ticks, keep_log)
        episode.reset(np.ascontiguousarray(solver.field(0, "XBAR")[:, 0]))
    if delay is not None:
        episode.set_latency(delay)
    if friction is not None:
        episode.set_friction(friction)
    if weight_scales is not None:
        solver.set_weight_scales(*weight_scales)
    if limits is not None:
        solver.set_limits(**limits)
    if plan_friction is not None:
        episode.plan_friction(plan_friction)
    out = dict(n_iters=[], n_ls_iters=[], n_reg_iters=[], cost=[], alive=[])
    for t in range(n_ticks):
        d, k = dist, None
        if kicks is not None and t in kicks:
            step, k = kicks[t]
            d = dataclasses.replace(dist if dist is not None else Disturbance(), kick_step=int(step))
        episode.advance(d, k)
        m = pd.update()
        phases, _ = builder.shift_solver_in_place(solver, phases, pd, m, ubar_mode="zero")
        if hook is not None:
            hook(t, phases)
        if plan_terrain:
            episode.plan_terrain()
        solver.solve(opt_rt)
        if post_hook is not None:
            post_hook(t, phases)
        ia = solver.info_arrays()
        out["n_iters"].append(ia["n_iters"]); out["n_ls_iters"].append(ia["n_ls_iters"]); out["n_reg_iters"].append(ia["n_reg_iters"]); out["cost"].append(ia["actual_cost"])
        out["alive"].append(episode.status()[1])
    res = {k: np.array(v) for k, v in out.items()}
    res["episode"] = episode; res["phases"] = phases
    return res
