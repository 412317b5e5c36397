"""Shared by tests/test_weights_host.py and tests/test_weights_gpu.py: per-problem cost-weight scales (include/hsddp_weights.h).

The reference.  The oracle has no per-problem weights, so a batch of B problems with scale rows is held against B SINGLE-problem handles of
liboracle_hsddp.so whose descriptors carry the numpy products q * sq_b, r * sr_b, qf * sqf_b (whole-body phases only): StackedOracle presents them
with the .field and step interface parity_common.run_steps / compare_solve take.

The scales.  scale_rows(B, seed): every coordinate of every row drawn from [0.25, 4] (log-uniform, so that a weight is as often halved as doubled),
different in every row; row 0 is all ones.

The emulator.  PwEmu runs the host build of the scaled programs (tests/_emu/pw_emu.cpp) behind the same interface: program WAVE = the one-wave
programs everywhere, QUAD = the lane-quad knot and terminal knot where the default launch uses them.
"""
import ctypes as C

import numpy as np

import walk_ref as wr
from conftest import pkg

DP = C.POINTER(C.c_double)
WAVE, QUAD = 0, 1
ROW = 84
MODEL_WB = 0

# the per-iterate cases of the issue: name -> (phase builder, seed of the initial states)
FLIGHT = dict(schedule=((1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1)), horizons=(1, 2, 3), last_next=(1, 1, 1, 1))
CASES = {
    "trot": (lambda: pkg.problems.wb_trot_problem(schedule=((1, 0, 0, 1), (0, 1, 1, 0)), horizons=(2, 3)), 20241222),
    "flight": (lambda: pkg.problems.wb_trot_problem(**FLIGHT), 31),
    "mhpc": (lambda: pkg.problems.mhpc_problem(wb_horizons=(3, 3), srb_schedule=((1, 0, 0, 1),), srb_horizons=(1,)), 20241222),
}
BATCHES = (1, 5, 17)
SCALE_SEED = 20260101


def scale_rows(batch, seed=SCALE_SEED):
    r = np.random.default_rng(seed)
    rows = np.exp(r.uniform(np.log(0.25), np.log(4.0), size=(batch, ROW)))
    rows[0] = 1.0
    return rows


def split(rows):
    return rows[:, :36], rows[:, 36:48], rows[:, 48:]


def scaled_phases(phases, row):
    """The phase list with q * sq, r * sr, qf * sqf in the descriptors of its whole-body phases (numpy products); everything else is shared."""
    out = []
    for p in phases:
        q = dict(p)
        d = type(p["desc"]).from_buffer_copy(p["desc"])
        if d.model == MODEL_WB:
            qv = np.array(d.q[:36]) * row[:36]; rv = np.array(d.r[:12]) * row[36:48]; fv = np.array(d.qf[:36]) * row[48:]
            for j in range(36):
                d.q[j] = qv[j]; d.qf[j] = fv[j]
            for j in range(12):
                d.r[j] = rv[j]
        q["desc"] = d
        out.append(q)
    return out


class StackedOracle:
    """B single-problem handles of one library behind the interface of a batch-B Solver.  heights: {phase: [B, 4]} puts row b's height into the
    ground_height of problem b's descriptor (the four legs of a row have to agree: ground_height is one number per descriptor)."""

    def __init__(self, lib, phases, x0, rows, heights=None):
        self.batch = x0.shape[0]
        self.phases = phases
        self.s = []
        for b in range(self.batch):
            ph = scaled_phases(phases, rows[b])
            for i, hts in (heights or {}).items():
                assert np.all(hts[b] == hts[b][0])
                ph[i]["desc"].ground_height = float(hts[b][0])
            s = pkg.Solver(lib, ph, batch=1)
            for i, p in enumerate(ph):
                X, U = np.asarray(p["Xbar"]), np.asarray(p["Ubar"])
                s.set_nominal(i, X[b:b + 1] if X.ndim == 3 else X, U[b:b + 1] if U.ndim == 3 else U)
            s.set_initial_condition(np.ascontiguousarray(x0[b:b + 1]))
            self.s.append(s)

    def _all(self, name, *a):
        return [getattr(s, name)(*a) for s in self.s]

    def hybrid_rollout(self, eps, opt): self._all("hybrid_rollout", eps, opt)
    def compute_cost(self, opt): self._all("compute_cost", opt)
    def LQ_approximation(self, opt): self._all("LQ_approximation", opt)
    def linear_rollout(self, eps, opt): self._all("linear_rollout", eps, opt)
    def update_nominal_trajectory(self): self._all("update_nominal_trajectory")
    def solve(self, opt): self._all("solve", opt)
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

    def set_initial_condition(self, x0):
        for b, s in enumerate(self.s):
            s.set_initial_condition(np.ascontiguousarray(x0[b:b + 1]))

    def close(self):
        self._all("close")


def build_emu(tmpdir):
    raw = wr.build_so(tmpdir, "pw_emu.cpp", "libhsddp_pw_emu.so")
    raw.pw_emu_hybrid_rollout.argtypes = [C.c_void_p, C.c_double, C.c_void_p, DP, C.c_int]
    raw.pw_emu_LQ_approximation.argtypes = [C.c_void_p, C.c_void_p, DP]
    raw.pw_emu_pack.argtypes = [DP, C.c_int, DP, C.c_int, C.c_int, C.c_int]
    raw.pw_emu_check_set.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    raw.pw_emu_check_range.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    return pkg._abi.bind(raw), raw


class PwEmu:
    """A batch-B handle of the lane emulator whose rollout and LQ steps run the scaled programs (rows [B, 84], None: the programs without the
    switch).  Everything else is the emulator's Solver."""

    def __init__(self, lib, raw, phases, x0, rows, program):
        self.raw, self.program = raw, program
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
        self.s = pkg.Solver(lib, phases, batch=x0.shape[0])
        for i, p in enumerate(phases):
            self.s.set_nominal(i, p["Xbar"], p["Ubar"])
        self.s.set_initial_condition(x0)

    def _rp(self):
        return None if self.rows is None else self.rows.ctypes.data_as(DP)

    def hybrid_rollout(self, eps, opt):
        assert self.raw.pw_emu_hybrid_rollout(self.s.h, float(eps), C.byref(opt), self._rp(), self.program) == 0

    def LQ_approximation(self, opt):
        assert self.raw.pw_emu_LQ_approximation(self.s.h, C.byref(opt), self._rp()) == 0

    def __getattr__(self, name):
        return getattr(self.s, name)


def make_hip(hip_lib, phases, x0, rows=None, **kw):
    """A batch-B handle of libhsddp_hip.so with the rows set through Solver.set_weight_scales."""
    s = pkg.Solver(hip_lib, phases, batch=x0.shape[0], **kw)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    if rows is not None:
        s.set_weight_scales(*split(rows))
    return s

