#!/usr/bin/env python3
"""Closed-loop policy simulation (include/hsddp_sim.h, kernel k_sim_quad): throughput beside the route the library had before; one JSON line.

  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve, --samples 16 perturbed initial states per
  problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0], resident on the device).  For n_steps in --windows (8, 50, 200):
    sim     hsddp_sim_run: kernel time (HIP events around the launch) and wall time of the call, median of --runs warm runs, as sample-knots per second
    chain   hsddp_hybrid_rollout(eps = 0, MS = 0) on the same handle, the one-wave single-shooting chain over the whole 200-knot horizon: wall time
            of the call, median of the same number of runs ALTERNATED with the sim runs of the 200-step window, as knots per second
  ratio = sim sample-knots/s over chain knots/s at the 200-step window: what the lane-quad mapping buys for this workload.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.
Kernel time alone: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/sim_bench.py --child --windows 200`, in a run of its own.

  python tools/sim_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--windows 8,50,200] [--timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    import torch
    torch.zeros(1, device=f"cuda:{args.device}")      # torch's HIP runtime up before the package's library is loaded
    import __graft_entry__ as ge
    pkg = ge.load_package()
    phases = pkg.problems.wb_trot_problem()
    B, R = args.batch, args.samples
    s = pkg.MultiPhaseDDP(phases, batch=B, device=args.device)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241220)
    s.set_initial_condition(x0)
    s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0))
    xb0 = s.field(0, "XBAR")[:, 0]
    # one set of R perturbations for every problem (the generator is a Python loop: B x R draws would dominate the tool's run time)
    d = pkg.problems.perturbed_states(np.zeros((1, 36)), R, 0.02, 0.2, seed=20241222)[0]
    xs = torch.from_numpy(np.ascontiguousarray(xb0[:, None, :] + d[None])).to(f"cuda:{args.device}")
    opt_ss = pkg.mhpc_ddp_setting(MS=0)
    n_wb = sum(p["desc"].horizon for p in phases)
    res = {"metric": "closed_loop_simulation", "kernel_source_hash": pkg.kernel_source_hash(), "batch": B, "samples": R, "solve_steps": args.steps,
           "waves": (B * R + 15) // 16, "windows": {}}
    windows = [int(w) for w in args.windows.split(",")]
    for n in windows:
        sim = pkg.Simulation(s, R, n)
        sim.run(xs)                                     # warm-up
        k_ms, w_ms, c_ms = [], [], []
        for _ in range(args.runs):
            t0 = time.perf_counter(); sim.run(xs); w_ms.append((time.perf_counter() - t0) * 1e3)
            k_ms.append(sim.kernel_time_ms())
            if n == max(windows):                       # the other route, alternated with the longest window
                t0 = time.perf_counter(); s.hybrid_rollout(0.0, opt_ss); c_ms.append((time.perf_counter() - t0) * 1e3)
        rows, _ = sim.rows()
        sim.close()
        km, wm = float(np.median(k_ms)), float(np.median(w_ms))
        e = {"kernel_ms": k_ms, "wall_ms": w_ms, "median_kernel_ms": km, "median_wall_ms": wm, "sample_knots": B * R * n,
             "sample_knots_per_s_kernel": B * R * n / (km * 1e-3), "sample_knots_per_s_wall": B * R * n / (wm * 1e-3),
             "diverged_samples": int((rows["first_bad"] >= 0).sum()), "max_dev_q": float(rows["dev_q"].max()), "min_height": float(rows["min_height"].min())}
        if c_ms:
            cm = float(np.median(c_ms[1:])) if len(c_ms) > 1 else float(c_ms[0])      # (the first call of the chain loads its code)
            e["chain"] = {"wall_ms": c_ms, "median_wall_ms": cm, "knots": B * n_wb, "knots_per_s": B * n_wb / (cm * 1e-3)}
            e["sim_over_chain"] = e["sample_knots_per_s_wall"] / e["chain"]["knots_per_s"]
        res["windows"][str(n)] = e
    s.close()
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--windows", default="8,50,200")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"sim_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
