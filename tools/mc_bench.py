#!/usr/bin/env python3
"""Disturbed closed-loop simulation (include/hsddp_mc.h, kernel k_sim_quad_mc): what each switch costs beside the plain run; one JSON line.

  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve, --samples 16 perturbed initial states per
  problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) and the kick array resident on the device, the whole --window (200 steps).  Variants:
    plain     hsddp_sim_run (k_sim_quad)
    umax      u_max 17 only
    su        sigma_u 0.2 only
    noise     sigma_u 0.2 + sigma_q 0.001 + sigma_v 0.01
    all       noise + u_max 17 + fall_height 0.16 + a kick of 0.3 on the base velocity y at step 10
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel
  time (HIP events around the launch) and wall time of the call, medians over the rounds, sample-knots per second, and the ratio of the kernel
  time to plain's.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.
Kernel names and times alone: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/mc_bench.py --child`, in a run of its own.

  python tools/mc_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--timeout 600]
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
    Dist = pkg.sim.Disturbance
    phases = pkg.problems.wb_trot_problem()
    B, R, n = args.batch, args.samples, args.window
    s = pkg.MultiPhaseDDP(phases, batch=B, device=args.device)
    s.set_initial_condition(pkg.problems.wb_ensemble_x0(B, 20241220))
    s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0))
    xb0 = s.field(0, "XBAR")[:, 0]
    # one set of R perturbations for every problem (the generator is a Python loop: B x R draws would dominate the tool's run time)
    d = pkg.problems.perturbed_states(np.zeros((1, 36)), R, 0.02, 0.2, seed=20241222)[0]
    xs = torch.from_numpy(np.ascontiguousarray(xb0[:, None, :] + d[None])).to(dev)
    kick = torch.zeros(B, R, 36, dtype=torch.float64, device=dev); kick[..., 19] = 0.3
    noise = dict(seed=20241222, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01)
    variants = [("plain", None, None), ("umax", Dist(seed=20241222, u_max=17.0), None), ("su", Dist(seed=20241222, sigma_u=0.2), None),
                ("noise", Dist(**noise), None), ("all", Dist(u_max=17.0, fall_height=0.16, kick_step=10, **noise), kick)]
    sim = pkg.Simulation(s, R, n)
    for _, dd, kk in variants:      # warm-up: code objects loaded, the disturbed run's buffers allocated
        sim.run(xs, dist=dd, kick=kk)
    k_ms = {v[0]: [] for v in variants}; w_ms = {v[0]: [] for v in variants}; stats = {}
    for rnd in range(args.runs):
        for name, dd, kk in variants:
            t0 = time.perf_counter(); sim.run(xs, dist=dd, kick=kk); w_ms[name].append((time.perf_counter() - t0) * 1e3)
            k_ms[name].append(sim.kernel_time_ms())
            if rnd == args.runs - 1:
                rows, _ = sim.rows()
                stats[name] = {"diverged_samples": int((rows["first_bad"] >= 0).sum()), "max_dev_q": float(rows["dev_q"].max()), "min_height": float(rows["min_height"].min()),
                               "max_torque": float(rows["max_torque"].max())}
                if dd is not None:
                    ex = sim.extra()
                    stats[name].update(n_sat=int(ex["n_sat"].sum()), fallen_samples=int((ex["first_fall"] >= 0).sum()))
    sim.close(); s.close()
    res = {"metric": "disturbed_closed_loop_simulation", "kernel_source_hash": pkg.kernel_source_hash(), "batch": B, "samples": R, "window": n, "solve_steps": args.steps,
           "waves": (B * R + 15) // 16, "runs": args.runs, "variants": {}}
    base = float(np.median(k_ms["plain"]))
    for name, _, _ in variants:
        km, wm = float(np.median(k_ms[name])), float(np.median(w_ms[name]))
        res["variants"][name] = {"kernel_ms": k_ms[name], "wall_ms": w_ms[name], "median_kernel_ms": km, "min_kernel_ms": float(min(k_ms[name])), "max_kernel_ms": float(max(k_ms[name])),
                                 "median_wall_ms": wm, "sample_knots_per_s_kernel": B * R * n / (km * 1e-3), "sample_knots_per_s_wall": B * R * n / (wm * 1e-3),
                                 "kernel_over_plain": km / base, **stats[name]}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window", type=int, default=200)
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
        print(f"mc_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
