#!/usr/bin/env python3
"""Per-problem tracking references (include/hsddp_refs.h): what they cost the solver and what hsddp_set_references costs; prints one JSON line.

  solve     config 3 (problems.wb_trot_problem(), WB N = 200, --batch 4096, --steps DDP iterations, cost_thresh 0): DDP it/s of a handle on the
            shared references and of one whose problems hold the same values per problem, alternated --reps times each (median).
  set       hsddp_set_references of every phase of the whole batch, host sources and device (torch) sources, at config 3 (WB, 4096 problems)
            and config 5 (problems.hkd_bound_problem(), HKD N = 200, 16 384 problems, fp32 handle): median wall time per call of the later
            calls (storage already per problem), algorithmic bytes (source read + raw arrays and the whole-body record written), GB/s.
Kernel time: run `rocprofv3 --kernel-trace --stats -- python tools/refs_bench.py --only set` and read k_pack_refs there.

  python tools/refs_bench.py [--batch 4096] [--steps 10] [--reps 3] [--calls 10] [--only solve|set]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as ge  # noqa: E402


def solve_rate(pkg, phases, x0, steps, per_problem):
    s = pkg.MultiPhaseDDP(phases, batch=x0.shape[0])
    if per_problem:
        for i, r in enumerate(pkg.problems.stack_references([phases] * x0.shape[0])):
            s.set_references(i, **r)
    s.set_initial_condition(x0)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=steps, cost_thresh=0.0)
    t0 = time.perf_counter(); s.solve(opt); dt = time.perf_counter() - t0
    info = s.info_arrays()
    s.close()
    return float(info["n_iters"].sum()) / dt, info


def set_bytes(phases, B):
    """Source read (the seven raw arrays of [B][h+1][width]) + the same written + the 80-double record of whole-body phases."""
    tot = 0
    for p in phases:
        n, m, py = pkg_dims[p["desc"].model]
        h1 = p["desc"].horizon + 1
        raw = B * h1 * ((n + m + py + 12 + 12 + 3) * 8 + 4 * 4)
        tot += 2 * raw + (B * h1 * 80 * 8 if p["desc"].model == 0 else 0)
    return tot


def time_set(pkg, phases, B, calls, device, precision):
    import torch
    s = pkg.MultiPhaseDDP(phases, batch=B, precision=precision)
    refs = pkg.problems.stack_references([phases] * 1)
    host = [{k: np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape[1:])) for k, v in r.items()} for r in refs]
    dev = [{k: torch.from_numpy(v).to(f"cuda:{device}") for k, v in r.items()} for r in host]
    out = {}
    for kind, src in (("host", host), ("device", dev)):
        t = []
        for c in range(calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, r in enumerate(src):
                s.set_references(i, **r)
            t.append(time.perf_counter() - t0)
        first, later = t[0], float(np.median(t[1:]))
        nbytes = set_bytes(phases, B)
        out[kind] = {"first_call_ms": first * 1e3, "median_ms": later * 1e3, "algorithmic_bytes": nbytes, "gbps_by_wall_time": nbytes / later / 1e9}
    ok = all(np.array_equal(s.get_references(i, B - 2, 2)[k], host[i][k][-2:]) for i in range(len(phases)) for k in host[i])
    s.close()
    out["read_back_equal"] = ok
    return out


pkg_dims = None


def main():
    global pkg_dims
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--hkd-batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--only", choices=["solve", "set"], default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device=f"cuda:{args.device}")      # torch's HIP runtime up before the package's library is loaded
    pkg = ge.load_package()
    pkg_dims = pkg._abi.MODEL_DIMS
    res = {"metric": "per_problem_references", "kernel_source_hash": pkg.kernel_source_hash()}
    wb = pkg.problems.wb_trot_problem()
    if args.only in (None, "solve"):
        x0 = pkg.problems.wb_ensemble_x0(args.batch, 20241220)
        solve_rate(pkg, wb, x0[:64], 2, True)                                   # warm-up (module load, first launches)
        rates = {"shared": [], "per_problem": []}
        infos = {}
        for r in range(args.reps):
            for kind in ("shared", "per_problem"):
                v, info = solve_rate(pkg, wb, x0, args.steps, kind == "per_problem")
                rates[kind].append(v); infos[kind] = info
        med = {k: float(np.median(v)) for k, v in rates.items()}
        res["solve"] = {"config": f"WB N=200 (4 x 50), batch {args.batch}, steps {args.steps}", "it_per_s": rates, "median_it_per_s": med,
                        "per_problem_over_shared": med["per_problem"] / med["shared"],
                        "same_iterations": bool(np.array_equal(infos["shared"]["n_iters"], infos["per_problem"]["n_iters"])),
                        "same_cost": bool(np.array_equal(infos["shared"]["actual_cost"], infos["per_problem"]["actual_cost"]))}
    if args.only in (None, "set"):
        res["set_config3"] = time_set(pkg, wb, args.batch, args.calls, args.device, pkg.PREC_F64)
        res["set_config5"] = time_set(pkg, pkg.problems.hkd_bound_problem(), args.hkd_batch, args.calls, args.device, pkg.PREC_F32)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
