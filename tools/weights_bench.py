#!/usr/bin/env python3
"""Per-problem cost-weight scales (include/hsddp_weights.h): what the _pw kernels cost a launch, and a demonstration study; one JSON line.

1. Per-launch times.  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096), a fixed-work solve of --steps DDP iterations after
   --warmup unmeasured solves (one AL iteration, cost_thresh 0).  Variants, ALTERNATED inside every round of --runs rounds in one process:
     unset    no table: k_rollout_quad / k_rollout_quad_term / k_rollout, k_lq - the launch sequence of a handle that never had scales
     ones     a table of 1.0: k_rollout_quad_pw / k_rollout_quad_term_pw / k_rollout_pw, k_lq_pw on the SAME iterates (q * 1.0 is q), so the two
              variants launch the same grids the same number of times and a launch is compared with its twin
     drawn    scales drawn per coordinate from [0.25, 4]: other iterates; listed for its counts and times, not compared launch by launch
   Before every solve the window is rebuilt without a warm start (hsddp_reconfigure, src_phase = -1), nominal trajectories and initial states are
   set again.  Per variant and launch name (hsddp_get_kernel_times: a rollout launch is the group quad kernel + quad terminal kernel + one-wave
   kernel that launch_rollout_list issues; k_ls_probe is the probe launch of the line search): launches and time per launch, median over the
   rounds; for `ones` the per-round ratio to `unset`.  There is no pass mark: the comparison is the twin in the same build.
2. Study.  3 x --study-group robots in one batch on the bound gait, the same start states in the three groups, the noise and the push of
   tools/latency_bench.py's study, sq on the twelve joint positions at 0.5 / 1 / 2, --study-ticks ticks of episode.run_mhpc with the scales set
   once: per group the robots that fell or diverged, the realised track_cost per step (the DESCRIPTORS' weights: the yardstick the groups share)
   and the largest dev_q.  One seed and a sample of --study-group robots per group: an illustration, not a result.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/weights_bench.py [--batch 4096] [--steps 20] [--warmup 5] [--runs 5] [--study-group 32] [--study-ticks 14] [--out FILE] [--timeout 900]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PAIRS = (("k_rollout", "k_rollout_pw"), ("k_lq", "k_lq_pw"), ("k_ls_probe", "k_ls_probe_pw"))


def launches(pkg, args):
    import numpy as np
    phases = pkg.problems.wb_trot_problem()
    B, nph = args.batch, len(phases)
    s = pkg.MultiPhaseDDP(phases, batch=B, device=args.device)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241220)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0)
    rng = np.random.default_rng(20260101)
    drawn = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=(B, 84))); drawn[0] = 1.0
    rows = {"unset": None, "ones": np.ones((B, 84)), "drawn": drawn}

    def solve(kind):
        s.reconfigure(phases, [-1] * nph, [0] * nph)
        for i, p in enumerate(phases):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(x0)
        if rows[kind] is None:
            s.clear_weight_scales()
        else:
            r = rows[kind]; s.set_weight_scales(r[:, :36], r[:, 36:48], r[:, 48:])
        s.lib.hsddp_reset_kernel_times(s.h)
        s.solve(opt)
        kt = s.kernel_times(64); ia = s.info_arrays()
        return {k: v for k, v in kt.items() if v[1] > 0}, int(ia["n_iters"].sum()), int(ia["n_ls_iters"].sum())
    for _ in range(args.warmup):
        for v in rows:
            solve(v)
    got = {v: [] for v in rows}
    for _ in range(args.runs):
        for v in rows:
            got[v].append(solve(v))
    out = {"batch": B, "knots": sum(p["desc"].horizon for p in phases), "solve_steps": args.steps, "warmup": args.warmup, "runs": args.runs, "variants": {}, "twins": {}}
    for v in rows:
        names = sorted(got[v][-1][0])
        out["variants"][v] = {"n_iters": got[v][-1][1], "n_ls_iters": got[v][-1][2],
                              "per_launch_ms": {n: float(np.median([g[0][n][0] / g[0][n][1] for g in got[v] if n in g[0]])) for n in names},
                              "launches": {n: got[v][-1][0][n][1] for n in names}}
    for a, b in PAIRS:
        if all(a in g[0] for g in got["unset"]) and all(b in g[0] for g in got["ones"]):
            ta = np.array([g[0][a][0] / g[0][a][1] for g in got["unset"]]); tb = np.array([g[0][b][0] / g[0][b][1] for g in got["ones"]])
            out["twins"][b] = {"twin": a, "twin_ms": float(np.median(ta)), "ms": float(np.median(tb)), "round_ratio_median": float(np.median(tb / ta)),
                               "round_ratio_min": float((tb / ta).min()), "round_ratio_max": float((tb / ta).max()),
                               "same_launch_count": got["unset"][-1][0][a][1] == got["ones"][-1][0][b][1]}
    s.close()
    return out


def study(pkg, G, ticks):
    import numpy as np
    import latency_bench as lb
    pd, phases, opt0, opt_rt, n = lb.bound_problem(pkg)
    B = 3 * G
    s = pkg.MultiPhaseDDP(phases, batch=B)
    x0 = np.ascontiguousarray(np.tile(lb.start_states(pkg, phases, G), (3, 1)))
    factor = np.repeat(np.array([0.5, 1.0, 2.0]), G)
    sq = np.ones((B, 36)); sq[:, 6:18] = factor[:, None]
    scales = (sq, np.ones((B, 12)), np.ones((B, 36)))
    s.set_weight_scales(*scales)
    e = s.episode(n, ticks); e.reset(x0); s.solve(opt0)
    dist = pkg.sim.Disturbance(seed=20241222, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1)
    kick = np.zeros((B, 36)); kick[:, 18] = 0.4; kick[:, 19] = 0.2
    pkg.episode.run_mhpc(s, pd, phases, opt_rt, ticks, dist=dist, kicks={3: (0, kick)}, episode=e, weight_scales=scales)
    rows, _ = e.rows()
    out = dict(batch=B, group=G, ticks=ticks, seeds=1, noise=dict(sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1),
               push="base velocity +0.4 x, +0.2 y at tick 3 step 0", scaled="sq[6:18] (joint positions)", per_group=[])
    for f in (0.5, 1.0, 2.0):
        r = rows[factor == f]
        out["per_group"].append(dict(sq_joint_positions=f, robots=int(len(r)), fell=int((r["end_reason"] == 2).sum()), diverged=int((r["end_reason"] == 1).sum()),
                                     track_cost_per_step=float((r["track_cost"] / np.maximum(r["steps"], 1)).mean()), max_dev_q=float(r["dev_q"].max())))
    e.close(); s.close()
    return out


def child(args):
    import torch
    torch.zeros(1, device=f"cuda:{args.device}")      # torch's HIP runtime up before the package's library is loaded
    import __graft_entry__ as ge
    pkg = ge.load_package()
    res = {"metric": "weight_scales", "kernel_source_hash": pkg.kernel_source_hash(), "per_launch": launches(pkg, args)}
    if args.study_group > 0:
        res["study"] = study(pkg, args.study_group, args.study_ticks)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--study-group", type=int, default=32)
    ap.add_argument("--study-ticks", type=int, default=14)      # (the trimmed reference of the fixture holds 16 ticks from window 11)
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"weights_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
