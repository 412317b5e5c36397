#!/usr/bin/env python3
"""Contact-force records (include/hsddp_grf.h; kernels k_sim_quad_grf, k_sim_quad_mc_grf, k_sim_quad_mc0_grf): what the records cost beside the
same run without them; one JSON line.

  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve, --samples 16 perturbed initial states per
  problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) resident on the device, the whole --window (200 steps).  Variants:
    plain / plain_grf     hsddp_sim_run, records off / on (mu 0.6, fz_min 0)
    umax / umax_grf       u_max 17 only (the walk without the generator)
    noise / noise_grf     sigma_u 0.2 + sigma_q 0.001 + sigma_v 0.01
    traj / traj_grf       hsddp_sim_run with keep_traj, at --traj-batch problems (the trajectories of the full batch do not fit)
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel
  time (HIP events around the launch) and wall time of the call, medians and min / max over the rounds, and for a records variant the ratio of
  its kernel time to its twin's.  The records of the last round are summarised (slipping samples, smallest fz and cone margin).

  The plain run of ANOTHER build of the library - the parent commit's, for "does the plain kernel cost what it cost" - is measured by the same
  tool: HSDDP_HIP_VARIANT=<name> python tools/grf_bench.py --only-plain (a library without the records' entry points has nothing else to measure),
  alternated with runs of this build by the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/grf_bench.py [--batch 4096] [--traj-batch 256] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--only-plain] [--timeout 600]
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
    sims = {"lean": pkg.Simulation(s, R, n)}
    variants = [("plain", "lean", None, False)]
    if not args.only_plain:
        noise = Dist(seed=20241222, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01)
        umax = Dist(seed=20241222, u_max=17.0)
        variants += [("plain_grf", "lean", None, True), ("umax", "lean", umax, False), ("umax_grf", "lean", umax, True), ("noise", "lean", noise, False),
                     ("noise_grf", "lean", noise, True)]
        if args.traj_batch > 0:
            # a second, smaller handle for the runs that keep trajectories
            Bt = min(args.traj_batch, B)
            st = pkg.MultiPhaseDDP(phases, batch=Bt, device=args.device)
            st.set_initial_condition(pkg.problems.wb_ensemble_x0(B, 20241220)[:Bt])
            st.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0))
            sims["traj"] = pkg.Simulation(st, R, n, keep_traj=True)
            xt = torch.from_numpy(np.ascontiguousarray(st.field(0, "XBAR")[:, 0][:, None, :] + d[None])).to(dev)
            variants += [("traj", "traj", None, False), ("traj_grf", "traj", None, True)]

    def run(name, which, dd, grf):
        sim = sims[which]
        if not args.only_plain:
            sim.set_grf(0.6 if grf else 0.0)
        x = xs if which == "lean" else xt
        t0 = time.perf_counter(); sim.run(x, dist=dd); w = (time.perf_counter() - t0) * 1e3
        return sim.kernel_time_ms(), w
    for v in variants:      # warm-up: code objects loaded, every buffer allocated
        run(*v)
    k_ms = {v[0]: [] for v in variants}; w_ms = {v[0]: [] for v in variants}; stats = {}
    for rnd in range(args.runs):
        for v in variants:
            k, w = run(*v)
            k_ms[v[0]].append(k); w_ms[v[0]].append(w)
            if rnd == args.runs - 1:
                sim = sims[v[1]]
                rows, _ = sim.rows()
                stats[v[0]] = {"diverged_samples": int((rows["first_bad"] >= 0).sum()), "max_torque": float(rows["max_torque"].max())}
                if v[3]:
                    g = sim.grf()
                    g = g[0] if isinstance(g, tuple) else g
                    stats[v[0]].update(slipping_samples=int((g["first_slip"] >= 0).sum()), pulling_samples=int((g["min_fz"] < 0).sum()), n_slip=int(g["n_slip"].sum()),
                                       min_fz=float(g["min_fz"].min()), min_cone=float(g["min_cone"].min()), max_fz=float(g["max_fz"].max()))
    for sim in sims.values():
        sim.close()
    res = {"metric": "contact_force_records", "kernel_source_hash": pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B,
           "traj_batch": 0 if args.only_plain else min(args.traj_batch, B), "samples": R, "window": n, "solve_steps": args.steps, "runs": args.runs, "variants": {}}
    for name, which, _, grf in variants:
        km, wm = float(np.median(k_ms[name])), float(np.median(w_ms[name]))
        nb = B if which == "lean" else min(args.traj_batch, B)
        res["variants"][name] = {"kernel_ms": k_ms[name], "wall_ms": w_ms[name], "median_kernel_ms": km, "min_kernel_ms": float(min(k_ms[name])), "max_kernel_ms": float(max(k_ms[name])),
                                 "median_wall_ms": wm, "sample_knots_per_s_kernel": nb * R * n / (km * 1e-3), **stats[name]}
        if grf:
            res["variants"][name]["kernel_over_twin"] = km / float(np.median(k_ms[name[:-4]]))
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--traj-batch", type=int, default=256, help="problems of the keep_traj variants (0: leave them out)")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--only-plain", action="store_true", help="the plain run alone, through the entry points every build of the library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"grf_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
