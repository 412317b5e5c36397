"""Cost of the policy latency of the MPC episodes (include/hsddp_latency.h) per tick, and a small closed-loop study of what a delay does.

    python tools/latency_bench.py [--batch 4096] [--reps 20] [--study-batch 96] [--study-ticks 14] [--out profiles/latency_bench.json]

The bound-gait fixture of the tests (tests/golden/cafe_tree, the builder advanced 11 MPC steps; n_exec = dt_mpc / dt_wb = 2).

1. Overhead.  Two episodes on ONE solved handle, one without latency and one with delay 2 for every robot (D = n_exec: the largest stash), advanced in
   turn in one process on the same window: per call the wall time of hsddp_episode_advance, and from the handle's kernel table the device time of
   k_episode_latency (HIP events around the launch).  Its traffic is 2 (n_exec + D) 516 x 8 bytes per robot - every row read once and written once.
   Medians over --reps calls after two warm-up calls.
2. Study.  --study-batch robots split evenly over the delays 0, 1 and 2, the same start state in the three groups, one noise setting and one push
   (a base velocity kick at tick 3), --study-ticks ticks of episode.run_mhpc: per delay the robots that fell or diverged and the mean realised
   tracking cost per executed step.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")
START_WINDOW = 11


def bound_problem(pkg):
    """(pd, phases, opt0, opt_rt, n_exec) of the bound gait, as tests/episode_common.py builds it."""
    from cafe_mpc_amd import builder
    cfg = builder.load_mhpc_config(TREE + "/MHPC/settings/mhpc_config.info")
    pd = builder.MHPCProblemData(builder.QuadReference(TREE + "/Reference/Data/bound/quad_reference.csv"), cfg,
                                 builder.load_cost_weights(TREE + "/" + cfg["costFile"]), builder.load_constraint_params(TREE + "/" + cfg["constraintParamFile"]))
    for _ in range(START_WINDOW):
        pd.update()
    phases, _ = pd.describe(ubar_mode="zero")
    opt0 = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info"); opt0.max_AL_iter, opt0.max_DDP_iter = 3, 4
    opt_rt = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info")
    opt_rt.max_AL_iter, opt_rt.max_DDP_iter = opt_rt.max_AL_iter_runtime, opt_rt.max_DDP_iter_runtime
    return pd, phases, opt0, opt_rt, int(round(float(cfg["dt_mpc"]) / cfg["dt_wb"]))


def start_states(pkg, phases, B, seed=20241222):
    x = np.repeat(phases[0]["Xbar"][:1], B, axis=0)
    out = pkg.problems.perturbed_states(x, 2, 0.002, 0.02, seed=seed)[:, 1]
    out[0] = x[0]
    return np.ascontiguousarray(out)


def overhead(pkg, B, reps):
    pd, phases, opt0, opt_rt, n = bound_problem(pkg)
    s = pkg.MultiPhaseDDP(phases, batch=B)
    x0 = start_states(pkg, phases, B)
    s.set_initial_condition(x0); s.solve(opt0)
    D = n
    off = s.episode(n, reps + 2); off.reset(x0)
    on = s.episode(n, reps + 2); on.set_latency(D); on.reset(x0)
    s.lib.hsddp_reset_kernel_times(s.h)
    t_off, t_on = [], []
    for i in range(reps + 2):
        t0 = time.perf_counter(); off.advance(); t1 = time.perf_counter(); on.advance(); t2 = time.perf_counter()
        if i >= 2:
            t_off.append((t1 - t0) * 1e3); t_on.append((t2 - t1) * 1e3)
    kt = s.kernel_times(64)
    lat_ms = kt["k_episode_latency"][0] / kt["k_episode_latency"][1]
    nbytes = 2 * (n + D) * 516 * 8 * B
    res = dict(batch=B, reps=reps, n_exec=n, D=D, advance_off_wall_ms=statistics.median(t_off), advance_on_wall_ms=statistics.median(t_on),
               latency_kernel_ms=lat_ms, latency_kernel_launches=kt["k_episode_latency"][1], commit_kernel_ms=kt["k_episode_commit"][0] / kt["k_episode_commit"][1],
               bytes_per_tick=nbytes, latency_kernel_gb_s=nbytes / (lat_ms * 1e-3) / 1e9, stale_steps=int(on.latency_rows()["n_stale"].sum()))
    res["overhead_wall_ms"] = res["advance_on_wall_ms"] - res["advance_off_wall_ms"]
    off.close(); on.close(); s.close()
    return res


def study(pkg, B, ticks):
    pd, phases, opt0, opt_rt, n = bound_problem(pkg)
    G = B // 3; B = 3 * G
    s = pkg.MultiPhaseDDP(phases, batch=B)
    x0 = np.ascontiguousarray(np.tile(start_states(pkg, phases, G), (3, 1)))
    delay = np.repeat(np.arange(3, dtype=np.int32), G)
    e = s.episode(n, ticks); e.reset(x0); s.solve(opt0)
    dist = pkg.sim.Disturbance(seed=20241222, sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1)
    kick = np.zeros((B, 36)); kick[:, 18] = 0.4; kick[:, 19] = 0.2
    pkg.episode.run_mhpc(s, pd, phases, opt_rt, ticks, dist=dist, kicks={3: (0, kick)}, episode=e, delay=delay)
    rows, _ = e.rows(); lr = e.latency_rows()
    out = dict(batch=B, ticks=ticks, noise=dict(sigma_u=0.1, sigma_q=1e-3, sigma_v=1e-2, u_max=30.0, fall_height=0.1), push="base velocity +0.4 x, +0.2 y at tick 3 step 0", per_delay=[])
    for d in range(3):
        r = rows[delay == d]
        out["per_delay"].append(dict(delay=d, robots=int(len(r)), fell=int((r["end_reason"] == 2).sum()), diverged=int((r["end_reason"] == 1).sum()),
                                     track_cost_per_step=float((r["track_cost"] / np.maximum(r["steps"], 1)).mean()), max_dev_q=float(r["dev_q"].max()),
                                     stale_steps=int(lr["n_stale"][delay == d].sum())))
    e.close(); s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--study-batch", type=int, default=96)
    ap.add_argument("--study-ticks", type=int, default=14)      # (the trimmed reference of the fixture holds 16 ticks from window 11)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = ge.load_package()
    res = dict(kernel_source_hash=pkg.kernel_source_hash(), overhead=overhead(pkg, a.batch, a.reps))
    print(json.dumps(res["overhead"]), file=sys.stderr)
    res["study"] = study(pkg, a.study_batch, a.study_ticks)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
