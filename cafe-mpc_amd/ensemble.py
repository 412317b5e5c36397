"""Schedule-candidate ensembles (include/hsddp_ensemble.h): S contact-schedule candidates, each one handle over the same batch of initial
states, solved side by side; a winner per state picked on the device; the winners' policies packed as MHPC_Command_lcmt words in one launch.

`select_rows` is the selection rule's specification; the device (csrc/ensemble.hpp ens_rank / ens_better) agrees with it bit for bit.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import Solver, PREC_F64

ROW_WORDS_PER_STEP = 1089      # HSDDP_CMD_WORDS_PER_STEP


def command_row_words(n_steps):
    return 1 + n_steps * ROW_WORDS_PER_STEP


def select_rows(rows, opt):
    """rows: [S, B, 8] result rows (launch.RESULT_FIELDS order: actual_cost, dyn_feas, max_tconstr, max_pconstr, n_iters, n_ls_iters,
    n_reg_iters, status); opt: the solve's option (its three feasibility thresholds).  Returns winner[B] (int32).

        violation = max(dyn_feas / dynamics_feas_thresh, max_tconstr / tconstr_thresh, max_pconstr / pconstr_thresh)
        tier 0: status in {0, 2} and violation <= 1     ordered by actual_cost
        tier 1: status in {0, 2} and violation >  1     ordered by violation, then actual_cost
        tier 2: any other status (1: regularisation failure), or a NaN among the four fp64 fields
        winner = first of the lowest non-empty tier, ties to the lowest candidate index

    Written as the scan the kernel performs (candidates in order, replace only on `strictly before`), with the same comparisons: the max is
    two `a > v` replacements, so both sides agree on every input, degenerate thresholds included."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 3 or rows.shape[2] != 8 or rows.shape[0] < 1:
        raise ValueError(f"rows must be [S, B, 8], got {rows.shape}")
    td, tt, tp = float(opt.dynamics_feas_thresh), float(opt.tconstr_thresh), float(opt.pconstr_thresh)
    with np.errstate(divide="ignore", invalid="ignore"):
        def rank(r):
            cost, dyn, tc, pc, status = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 7].astype(np.int64)
            v = dyn / td
            a = tc / tt
            v = np.where(a > v, a, v)
            a = pc / tp
            v = np.where(a > v, a, v)
            nan = np.isnan(cost) | np.isnan(dyn) | np.isnan(tc) | np.isnan(pc)
            tier = np.where(nan | ((status != 0) & (status != 2)), 2, np.where(v <= 1.0, 0, 1))
            return cost, v, tier

        def better(a, b):
            (ca, va, ta), (cb, vb, tb) = a, b
            return np.where(ta != tb, ta < tb,
                            np.where(ta == 0, ca < cb, np.where(ta == 1, (va < vb) | ((va == vb) & (ca < cb)), False)))

        best = rank(rows[0])
        winner = np.zeros(rows.shape[1], dtype=np.int32)
        for c in range(1, rows.shape[0]):
            r = rank(rows[c])
            take = better(r, best)
            winner = np.where(take, c, winner).astype(np.int32)
            best = tuple(np.where(take, x, y) for x, y in zip(r, best))
    return winner


def info_rows(info):
    """hsddp_info_t array (ctypes) -> [n, 8] fp64 rows in launch.RESULT_FIELDS order."""
    return np.array([[i.actual_cost, i.dyn_feas, i.max_tconstr, i.max_pconstr, i.n_iters, i.n_ls_iters, i.n_reg_iters, i.status] for i in info],
                    dtype=np.float64).reshape(len(info), 8)


class ScheduleEnsemble:
    """S schedule candidates over one batch of initial states on one device, through libhsddp_hip.so's ensemble entry points.

    candidates: list of phase lists (problems.py builders); one handle per candidate.  batch: int (every candidate) or one int per candidate
    (the sharded path: a rank's segments differ in length; `select` needs equal batches).  There is no per-handle fallback: the library must
    export include/hsddp_ensemble.h."""

    def __init__(self, candidates, batch, device=0, precision=PREC_F64, lib=None):
        if lib is None:
            from . import load_hip_library
            lib = load_hip_library()
        self.lib = _abi.bind_ensemble(lib)
        batches = [int(batch)] * len(candidates) if np.isscalar(batch) else [int(b) for b in batch]
        if len(batches) != len(candidates) or not candidates:
            raise ValueError("one batch per candidate")
        self.batches, self.device = batches, device
        self.solvers = []
        for phases, b in zip(candidates, batches):
            s = Solver(lib, phases, batch=b, device=device, precision=precision)
            for i, p in enumerate(phases):
                s.set_nominal(i, p["Xbar"], p["Ubar"])
            self.solvers.append(s)
        hs = (C.c_void_p * len(self.solvers))(*[s.h.value for s in self.solvers])
        self.e = C.c_void_p()
        rc = self.lib.hsddp_ensemble_create(C.byref(self.e), len(self.solvers), hs)
        if rc != 0:
            raise RuntimeError(f"hsddp_ensemble_create failed rc={rc}")

    @property
    def n_cands(self):
        return len(self.solvers)

    def close(self):
        if getattr(self, "e", None):
            self.lib.hsddp_ensemble_destroy(self.e)
            self.e = C.c_void_p()
        for s in getattr(self, "solvers", []):
            s.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}")

    def set_initial_condition(self, x0):
        """x0 [batch, n]: the same states for every candidate (or a list of one array per candidate)."""
        for i, s in enumerate(self.solvers):
            s.set_initial_condition(x0[i] if isinstance(x0, (list, tuple)) else x0)

    def solve(self, opt, max_cputime_ms=1e6, concurrent=True):
        self._ck(self.lib.hsddp_ensemble_solve(self.e, C.byref(opt), C.c_float(max_cputime_ms), 1 if concurrent else 0), "hsddp_ensemble_solve")

    def rows(self):
        """[S, B, 8] result rows of every candidate (hsddp_get_info); needs equal batches."""
        return np.stack([info_rows(s.get_info()) for s in self.solvers])

    def select(self, opt):
        """(winner[B] int32, best_rows[B, 8]): the device's pick per state and the winner's result row."""
        B = self.batches[0]
        w = np.zeros(B, dtype=np.int32)
        best = (_abi.Info * B)()
        self._ck(self.lib.hsddp_ensemble_select(self.e, C.byref(opt), w.ctypes.data_as(_abi.IP), best), "hsddp_ensemble_select")
        return w, info_rows(best)

    def export_mpc_commands(self, pairs, n_steps=8, mpc_time=0.0, dt=0.01, status_times=None, out=None):
        """MHPC_Command_lcmt words of (candidate, problem) pairs, one row each ([n, 1 + n_steps*1089]); row i is bit-identical to the
        candidate's own export_mpc_command(problem).  status_times: None or one [n_phases, 4] array (or None) per candidate.
        out: None -> host numpy uint32 array; a torch int32 tensor of that shape on this ensemble's device (or a raw device address of
        n * (1 + n_steps*1089) words there) -> written in place (the words' bit patterns) and returned."""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        n = pairs.shape[0]
        cand, prob = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        st_keep, st_ptrs = [], None
        if status_times is not None:
            st_ptrs = (C.c_void_p * self.n_cands)()
            for i, st in enumerate(status_times):
                if st is not None:
                    a = np.ascontiguousarray(st, dtype=np.float32)
                    assert a.shape == (len(self.solvers[i].phases), 4)
                    st_keep.append(a); st_ptrs[i] = a.ctypes.data
        W = command_row_words(n_steps)
        if out is None:
            host = np.zeros((n, W), dtype=np.uint32)
            dst, dev = host.ctypes.data, 0
        elif isinstance(out, int):              # a raw device address of n * W words on this ensemble's device
            host, dst, dev = None, out, 1
        else:
            assert tuple(out.shape) == (n, W) and out.is_contiguous() and out.element_size() == 4 and out.device.type == "cuda"
            host, dst, dev = None, out.data_ptr(), 1
        self._ck(self.lib.hsddp_ensemble_export_mpc_commands(self.e, n, cand.ctypes.data_as(_abi.IP), prob.ctypes.data_as(_abi.IP), n_steps,
                                                             float(mpc_time), float(dt), st_ptrs, dst, dev), "hsddp_ensemble_export_mpc_commands")
        return host if out is None else out
