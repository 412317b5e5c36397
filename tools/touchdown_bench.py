#!/usr/bin/env python3
"""Per-problem touchdown heights (include/hsddp_touchdown.h): what the _tdh rollout kernels cost a solve, and what k_td_terrain costs; one JSON line.

  The benchmark shape: config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096), a fixed-work solve of --steps DDP iterations (one AL
  iteration, cost_thresh 0).  Variants:
    unset    no phase has heights of its own: launch_rollout_list launches k_rollout_quad_term / k_rollout - the launch sequence of the parent commit
    shared   every phase with a touchdown constraint has heights equal to its ground_height: k_rollout_quad_term_tdh / k_rollout_tdh, the same solve
  --runs rounds; in every round each variant solves once, in the order above, so the variants are ALTERNATED in one session.  Before every solve the
  window is rebuilt without a warm start (hsddp_reconfigure, src_phase = -1: trajectories and AL / ReB parameters as created), the nominal
  trajectories and initial states are set again, and - for `shared` - the heights: every solve starts from the same state.  Per variant: wall time
  of hsddp_solve and the handle's own solve time, median and min / max over the rounds; for `shared` the per-round ratio to `unset`.
  k_td_terrain: --runs calls of hsddp_touchdown_from_terrain from a DEVICE grid (64 maps of 64 x 64 cells, a map drawn per problem), the kernel's
  time from the handle's event pairs.

  The `unset` row of ANOTHER build of the library - the parent commit's - is measured by the same tool: HSDDP_HIP_VARIANT=<name> python
  tools/touchdown_bench.py --only-parent (a library without the entry points has nothing else to measure), alternated with runs of this build by
  the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/touchdown_bench.py [--batch 4096] [--steps 10] [--runs 5] [--only-parent] [--timeout 600]
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
    dev = f"cuda:{args.device}"
    torch.zeros(1, device=dev)      # torch's HIP runtime up before the package's library is loaded
    import __graft_entry__ as ge
    pkg = ge.load_package()
    phases = pkg.problems.wb_trot_problem()
    B, nph = args.batch, len(phases)
    s = pkg.MultiPhaseDDP(phases, batch=B, device=args.device)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241220)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0)
    td = [i for i, p in enumerate(phases) if pkg.problems.touchdown_legs(p["desc"]).any()]
    variants = ["unset"] if args.only_parent else ["unset", "shared"]

    def solve(kind):
        s.reconfigure(phases, [-1] * nph, [0] * nph)
        for i, p in enumerate(phases):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(x0)
        if kind == "shared":
            for i in td:
                s.set_touchdown_heights(i, np.full((B, 4), phases[i]["desc"].ground_height))
        t0 = time.perf_counter(); s.solve(opt); wall = (time.perf_counter() - t0) * 1e3
        ia = s.info_arrays()
        return wall, float(ia["solve_time_ms"][0]) if "solve_time_ms" in ia else None, int(ia["n_iters"].sum()), int(ia["n_ls_iters"].sum()), float(ia["actual_cost"].sum())
    for v in variants:      # warm-up: code objects loaded, every buffer allocated
        solve(v)
    rows = {v: [] for v in variants}
    for _ in range(args.runs):
        for v in variants:
            rows[v].append(solve(v))
    variant = bool(os.environ.get("HSDDP_HIP_VARIANT", ""))
    res = {"metric": "touchdown", "kernel_source_hash": None if variant else pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B,
           "solve_steps": args.steps, "runs": args.runs, "touchdown_phases": td, "variants": {}}
    for v in variants:
        w = np.array([r[0] for r in rows[v]])
        res["variants"][v] = {"solve_wall_ms": w.tolist(), "median_ms": float(np.median(w)), "min_ms": float(w.min()), "max_ms": float(w.max()),
                              "n_iters": rows[v][-1][2], "n_ls_iters": rows[v][-1][3], "cost_sum": rows[v][-1][4]}
    if not args.only_parent:
        q = np.array([r[0] for r in rows["shared"]]) / np.array([r[0] for r in rows["unset"]])
        res["variants"]["shared"].update(round_ratio_median=float(np.median(q)), round_ratio_min=float(q.min()), round_ratio_max=float(q.max()),
                                         same_counts=rows["shared"][-1][2:4] == rows["unset"][-1][2:4])
        rng = np.random.default_rng(20241222)
        H = torch.from_numpy(0.01 * rng.standard_normal((64, 64, 64))).to(dev)
        mo = torch.from_numpy(rng.integers(0, 64, size=B).astype(np.int32)).to(dev)
        ter = pkg.sim.Terrain(H=H, x0=-1.1, y0=-1.6, cx=0.05, cy=0.05)
        s.plan_terrain(ter, mo)
        k0 = s.kernel_times().get("k_td_terrain", (0.0, 0))
        ms = []
        for _ in range(args.runs):
            s.plan_terrain(ter, mo)
            k1 = s.kernel_times().get("k_td_terrain", (0.0, 0))
            ms.append((k1[0] - k0[0]) / max(k1[1] - k0[1], 1)); k0 = k1
        res["k_td_terrain"] = {"lanes": nph * B * 4, "kernel_ms": ms, "median_kernel_ms": float(np.median(ms)), "min_kernel_ms": float(min(ms)), "max_kernel_ms": float(max(ms))}
    s.close()
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--only-parent", action="store_true", help="the row without heights alone, through the entry points the parent commit's library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"touchdown_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
