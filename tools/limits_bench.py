#!/usr/bin/env python3
"""Per-problem constraint limits (include/hsddp_limits.h): what the _lim kernels cost a launch, and a demonstration study; one JSON line.

1. Per-launch times.  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096), a fixed-work solve of --steps DDP iterations after
   --warmup unmeasured solves (one AL iteration, cost_thresh 0).  Variants, ALTERNATED inside every round of --runs rounds in one process:
     parent   the PARENT commit's library (--parent NAME: cafe-mpc_amd/variants/libhsddp_hip_NAME.so, a `make variant` build of the parent's sources;
              left out when the file is not there), no table: k_rollout_quad / k_rollout_quad_term / k_rollout, k_lq
     unset    this library, no table: the same launch sequence - the code objects are the parent's (tests/test_weights_host.py holds their hashes)
     nan      this library, a table whose every entry is NaN: k_rollout_quad_lim / k_rollout_quad_term / k_rollout_lim, k_lq_lim on the SAME iterates
              (every resolved entry is the descriptor's value, the scale table is ones), so the variants launch the same grids the same number of
              times and a launch is compared with its twin
   Before every solve the window is rebuilt without a warm start (hsddp_reconfigure, src_phase = -1), nominal trajectories and initial states are
   set again.  Per variant and launch name (hsddp_get_kernel_times: a rollout launch is the group quad kernel + quad terminal kernel + one-wave
   kernel that launch_rollout_list issues; k_ls_probe is the probe launch of the line search): launches and time per launch, median over the
   rounds; for `nan` the per-round ratio to `unset` and to `parent` (median, min, max), and for `unset` the per-round ratio to `parent` - two runs
   of identical code objects, i.e. the spread a ratio has to exceed to mean anything.  There is no pass mark.
2. Study.  3 x --study-group robots in one episode on the bound gait, all on ground with mu_s = --study-mu (one friction row), the same start states
   in the three groups, the noise and the push of tools/latency_bench.py's study.  Group 0 plans with the descriptor's mu, group 1 with what
   Episode.plan_friction(1.0) wrote and group 2 with what plan_friction(0.7) wrote (both columns are read back and put into one table, NaN for group
   0).  Per group: sliding onsets (friction_rows, summed over the ticks), robots that fell or diverged, the realised track_cost per step.  One seed
   and a few dozen robots per group: a demonstration of the mechanism, not a tuning result.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/limits_bench.py [--batch 4096] [--steps 20] [--warmup 3] [--runs 5] [--parent parent] [--study-group 32] [--study-ticks 14] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PAIRS = (("k_rollout", "k_rollout_lim"), ("k_lq", "k_lq_lim"), ("k_ls_probe", "k_ls_probe_lim"))


def launches(pkg, args):
    import numpy as np
    phases = pkg.problems.wb_trot_problem()
    B, nph = args.batch, len(phases)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241220)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0)
    this = pkg.load_hip_library()
    ppath = os.path.join(os.path.dirname(pkg.HIP_LIB_PATH), "variants", f"libhsddp_hip_{args.parent}.so")
    solvers = {}
    if args.parent and os.path.exists(ppath):
        solvers["parent"] = pkg.Solver(pkg._abi.bind(ctypes.CDLL(ppath)), phases, batch=B, device=args.device)
    solvers["unset"] = pkg.Solver(this, phases, batch=B, device=args.device)
    solvers["nan"] = pkg.Solver(this, phases, batch=B, device=args.device)
    solvers["nan"].set_limits(mu=np.full(B, np.nan))

    def solve(kind):
        s = solvers[kind]
        s.reconfigure(phases, [-1] * nph, [0] * nph)
        for i, p in enumerate(phases):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(x0)
        s.lib.hsddp_reset_kernel_times(s.h)
        s.solve(opt)
        kt = s.kernel_times(64); ia = s.info_arrays()
        return {k: v for k, v in kt.items() if v[1] > 0}, int(ia["n_iters"].sum()), int(ia["n_ls_iters"].sum())
    for _ in range(args.warmup):
        for v in solvers:
            solve(v)
    got = {v: [] for v in solvers}
    for _ in range(args.runs):
        for v in solvers:
            got[v].append(solve(v))
    out = {"batch": B, "knots": sum(p["desc"].horizon for p in phases), "solve_steps": args.steps, "warmup": args.warmup, "runs": args.runs, "variants": {}, "twins": {},
           "same_iterates": len({(got[v][-1][1], got[v][-1][2]) for v in solvers}) == 1}
    for v in solvers:
        names = sorted(got[v][-1][0])
        out["variants"][v] = {"n_iters": got[v][-1][1], "n_ls_iters": got[v][-1][2],
                              "per_launch_ms": {n: float(np.median([g[0][n][0] / g[0][n][1] for g in got[v] if n in g[0]])) for n in names},
                              "launches": {n: got[v][-1][0][n][1] for n in names}}

    def ratio(num, nn, den, dn):
        ta = np.array([g[0][dn][0] / g[0][dn][1] for g in got[den]]); tb = np.array([g[0][nn][0] / g[0][nn][1] for g in got[num]])
        return {"ms": float(np.median(tb)), "twin_ms": float(np.median(ta)), "twin_ms_min": float(ta.min()), "twin_ms_max": float(ta.max()), "round_ratio_median": float(np.median(tb / ta)),
                "round_ratio_min": float((tb / ta).min()), "round_ratio_max": float((tb / ta).max()), "same_launch_count": got[den][-1][0][dn][1] == got[num][-1][0][nn][1]}
    for a, b in PAIRS:
        if not (all(a in g[0] for g in got["unset"]) and all(b in g[0] for g in got["nan"])):
            continue
        out["twins"][b] = {"twin": a, "vs_unset": ratio("nan", b, "unset", a)}
        if "parent" in solvers:
            out["twins"][b]["vs_parent"] = ratio("nan", b, "parent", a)
            out["twins"][b]["unset_vs_parent"] = ratio("unset", a, "parent", a)
    for s in solvers.values():
        s.close()
    return out


def study(pkg, G, ticks, mu_s):
    import numpy as np
    import latency_bench as lb
    pd, phases, opt0, opt_rt, n = lb.bound_problem(pkg)
    B = 3 * G
    s = pkg.MultiPhaseDDP(phases, batch=B)
    x0 = np.ascontiguousarray(np.tile(lb.start_states(pkg, phases, G), (3, 1)))
    group = np.repeat(np.arange(3), G)
    e = s.episode(n, ticks); e.reset(x0)
    e.set_substeps(4); e.set_grf(0.6); e.set_contact(-3.0, 0.0); e.set_friction(pkg.sim.Friction(mu=[[mu_s, 0.8 * mu_s]], v_stick=0.02))
    e.plan_friction(0.7); m07 = s.limits(0)["mu"]
    e.plan_friction(1.0); m10 = s.limits(0)["mu"]
    mu = np.where(group == 0, np.nan, np.where(group == 1, m10, m07))
    s.set_limits(mu=mu)
    s.solve(opt0)
    dist = pkg.sim.Disturbance(seed=20241222, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1)
    kick = np.zeros((B, 36)); kick[:, 18] = 0.4; kick[:, 19] = 0.2
    onsets = np.zeros(B, dtype=np.int64); slides = np.zeros(B, dtype=np.int64)

    def hook(t, ph):
        f = e.friction_rows(); onsets[:] += f["n_onset"]; slides[:] += f["n_slide"]
    pkg.episode.run_mhpc(s, pd, phases, opt_rt, ticks, dist=dist, kicks={3: (0, kick)}, episode=e, hook=hook)
    rows, _ = e.rows()
    out = dict(batch=B, group=G, ticks=ticks, seeds=1, ground_mu_s=mu_s, noise=dict(sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1),
               push="base velocity +0.4 x, +0.2 y at tick 3 step 0", per_group=[])
    for g, name in enumerate(("descriptor", "plan_friction(1.0)", "plan_friction(0.7)")):
        r = rows[group == g]; plan = s.limits(0)["mu"][group == g]
        out["per_group"].append(dict(plans_with=name, planner_mu=float(plan[0]), robots=int(len(r)), sliding_onsets=int(onsets[group == g].sum()), sliding_steps=int(slides[group == g].sum()),
                                     fell=int((r["end_reason"] == 2).sum()), diverged=int((r["end_reason"] == 1).sum()),
                                     track_cost_per_step=float((r["track_cost"] / np.maximum(r["steps"], 1)).mean()), max_dev_q=float(r["dev_q"].max())))
    e.close(); s.close()
    return out


def child(args):
    import torch
    torch.zeros(1, device=f"cuda:{args.device}")      # torch's HIP runtime up before the package's library is loaded
    import __graft_entry__ as ge
    pkg = ge.load_package()
    res = {"metric": "constraint_limits", "kernel_source_hash": pkg.kernel_source_hash()}
    if args.runs > 0:
        res["per_launch"] = launches(pkg, args)
    if args.study_group > 0:
        res["study"] = study(pkg, args.study_group, args.study_ticks, args.study_mu)
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent", default="parent")
    ap.add_argument("--study-group", type=int, default=32)
    ap.add_argument("--study-ticks", type=int, default=14)      # (the trimmed reference of the fixture holds 16 ticks from window 11)
    ap.add_argument("--study-mu", type=float, default=0.3)
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
        print(f"limits_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
