"""Closed-loop rollouts of a solved whole-body policy from perturbed initial states (include/hsddp_sim.h; libhsddp_hip.so only).

    x0 = problems.perturbed_states(solver.field(0, "XBAR")[:, 0], 16, 0.02, 0.2, seed=1)      # [B, 16, 36]
    res = solver.simulate(x0, n_steps=50)              # one-off: creates, runs, reads back, destroys
    res["rows"]["dev_q"], res["rows"]["first_bad"], res["x_final"]

    sim = Simulation(solver, n_samples=16, n_steps=50)  # kept across ticks: run() makes no device allocation
    sim.run(x0); rows, x_final = sim.rows()

Nothing here computes anything: the rollout is the k_sim_quad kernel (csrc/wb_sim.hpp)."""
import ctypes as C

import numpy as np

from . import _abi


class Simulation:
    """One hsddp_sim_t on a Solver's handle.  Stale after Solver.reconfigure (run raises; create a new one).  Close it before the solver."""

    def __init__(self, solver, n_samples, n_steps, keep_traj=False):
        self.lib = _abi.bind_sim(solver.lib)      # raises on a library without include/hsddp_sim.h (the CPU checker)
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

    def run(self, x0):
        """x0: [B, R, 36] float64, a numpy array (copied) or a contiguous torch tensor on the handle's device (read in place)."""
        shape = (self.solver.batch, self.R, 36)
        if type(x0).__module__.startswith("torch"):
            import torch
            if x0.dtype != torch.float64 or not x0.is_contiguous() or x0.device.type != "cuda" or tuple(x0.shape) != shape:
                raise ValueError(f"x0: need a contiguous float64 tensor of shape {shape} on the handle's device, got {x0.dtype} {tuple(x0.shape)} on {x0.device}")
            torch.cuda.current_stream(x0.device).synchronize()      # the kernel runs on the handle's stream
            rc = self.lib.hsddp_sim_run(self.s, x0.data_ptr(), 1)
        else:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != shape:
                raise ValueError(f"x0: shape {x0.shape}, need {shape}")
            rc = self.lib.hsddp_sim_run(self.s, x0.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"hsddp_sim_run failed rc={rc}")

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


def simulate(solver, x0, n_steps, keep_traj=False):
    """One-off simulation on `solver`: dict with rows, x_final and, with keep_traj, X and U (see Simulation)."""
    sim = Simulation(solver, x0.shape[1], n_steps, keep_traj)
    try:
        sim.run(x0)
        rows, xf = sim.rows()
        out = dict(rows=rows, x_final=xf)
        if keep_traj:
            out["X"], out["U"] = sim.traj()
        return out
    finally:
        sim.close()
