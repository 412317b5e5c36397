#!/usr/bin/env python3
"""Sub-stepped integration (include/hsddp_substep.h; the six k_sim_quad*_sub kernels): what S substeps per control knot cost beside the same run
with one; one JSON line.

  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve, --samples 16 perturbed initial states per
  problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) resident on the device, the whole --window (200 steps).  Variants:
    plain_s1 / _s2 / _s4 / _s8     hsddp_sim_run at S = 1, 2, 4, 8
    noise_s1 / noise_s4            case D's switches: sigma_u 0.2 + sigma_q 0.001 + sigma_v 0.01 + u_max 8 + fall_height 0.16
    grf_s1 / grf_s4                hsddp_sim_run with the contact-force records on (mu 0.6, fz_min 0)
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel
  time (HIP events around the launch) and wall time of the call, medians and min / max over the rounds, and for S > 1 the ratio of its kernel
  time to the S = 1 row of the same kind.  The last round is summarised (diverged samples, largest torque, the records' counters, and the
  largest distance of the final states from the S = 1 run's).

  The S = 1 rows of ANOTHER build of the library - the parent commit's, for "does a run with one substep cost what it cost" - are measured by
  the same tool: HSDDP_HIP_VARIANT=<name> python tools/substep_bench.py --only-s1 (a library without the substep entry points has nothing else
  to measure), alternated with runs of this build by the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/substep_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--only-s1] [--timeout 600]
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
    sim = pkg.Simulation(s, R, n)
    noise = Dist(seed=20241222, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01, u_max=8.0, fall_height=0.16)
    # (name, kind, S, disturbance, records)
    variants = [("plain_s1", "plain", 1, None, False), ("noise_s1", "noise", 1, noise, False), ("grf_s1", "grf", 1, None, True)]
    if not args.only_s1:
        variants = [("plain_s1", "plain", 1, None, False), ("plain_s2", "plain", 2, None, False), ("plain_s4", "plain", 4, None, False), ("plain_s8", "plain", 8, None, False),
                    ("noise_s1", "noise", 1, noise, False), ("noise_s4", "noise", 4, noise, False), ("grf_s1", "grf", 1, None, True), ("grf_s4", "grf", 4, None, True)]

    def run(name, kind, S, dd, grf):
        if not args.only_s1:
            sim.set_substeps(S)
        sim.set_grf(0.6 if grf else 0.0)
        t0 = time.perf_counter(); sim.run(xs, dist=dd); w = (time.perf_counter() - t0) * 1e3
        return sim.kernel_time_ms(), w
    for v in variants:      # warm-up: code objects loaded, every buffer allocated
        run(*v)
    k_ms = {v[0]: [] for v in variants}; w_ms = {v[0]: [] for v in variants}; stats = {}; finals = {}
    for rnd in range(args.runs):
        for v in variants:
            k, w = run(*v)
            k_ms[v[0]].append(k); w_ms[v[0]].append(w)
            if rnd == args.runs - 1:
                rows, xf = sim.rows()
                finals[v[0]] = xf
                ok = rows["first_bad"] < 0
                stats[v[0]] = {"diverged_samples": int((~ok).sum()), "max_torque": float(rows["max_torque"].max()), "min_height": float(rows["min_height"][ok].min())}
                if v[3] is not None:
                    e = sim.extra()
                    stats[v[0]].update(fallen_samples=int((e["first_fall"] >= 0).sum()), n_sat=int(e["n_sat"].sum()))
                if v[4]:
                    g = sim.grf()
                    stats[v[0]].update(slipping_samples=int((g["first_slip"] >= 0).sum()), pulling_samples=int((g["min_fz"] < 0).sum()), n_slip=int(g["n_slip"].sum()),
                                       min_fz=float(g["min_fz"].min()), min_cone=float(g["min_cone"].min()), max_fz=float(g["max_fz"].max()))
    sim.close()
    # the hash names the sources of THIS tree: it says nothing about a variant library, which is another build (the parent commit's, say)
    variant = bool(os.environ.get("HSDDP_HIP_VARIANT", ""))
    res = {"metric": "substepped_integration", "kernel_source_hash": None if variant else pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B, "samples": R,
           "window": n, "solve_steps": args.steps, "runs": args.runs, "variants": {}}
    for name, kind, S, _, _ in variants:
        km, wm = float(np.median(k_ms[name])), float(np.median(w_ms[name]))
        res["variants"][name] = {"substeps": S, "kernel_ms": k_ms[name], "wall_ms": w_ms[name], "median_kernel_ms": km, "min_kernel_ms": float(min(k_ms[name])),
                                 "max_kernel_ms": float(max(k_ms[name])), "median_wall_ms": wm, "sample_knots_per_s_kernel": B * R * n / (km * 1e-3), **stats[name]}
        if S > 1:
            both = (np.isfinite(finals[name]) & np.isfinite(finals[kind + "_s1"])).all(axis=-1)
            res["variants"][name]["kernel_over_s1"] = km / float(np.median(k_ms[kind + "_s1"]))
            res["variants"][name]["max_final_state_distance_from_s1"] = float(np.abs(finals[name][both] - finals[kind + "_s1"][both]).max())
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
    ap.add_argument("--only-s1", action="store_true", help="the S = 1 rows alone, through the entry points every build of the library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"substep_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
