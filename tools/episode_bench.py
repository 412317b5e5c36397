"""Cost of one MPC-episode tick (include/hsddp_episode.h) beside the solve, and the same tick done through the calls that existed before it.

    python tools/episode_bench.py [--batch 4096] [--reps 20] [--out profiles/r08ep_episode_bench.json]

Config 3's window (whole-body trot, 4 x 50 knots), every problem one robot.  Two tick lengths on the same window: n_exec = 50 ends inside the
schedule without a touchdown (walk + commit), n_exec = 100 ends exactly on the touchdown of the second phase (walk + commit + pending reset
map).  Per call the wall time of hsddp_episode_advance (it returns with the results in place) and the device time of each of its kernels (HIP
events around the launch): the walk's from the simulation object, k_episode_commit and k_episode_impact from the handle's kernel table; what
remains of the wall time is host work, launches and the synchronisation.  The baseline is what a caller had to do per tick before: a simulation object
created, run from host states, the final states read back, hsddp_set_initial_condition, the object destroyed.  With one sample per problem a
launch of the walk has batch / 16 waves: below 16 384 problems it does not fill the card's 1 024 SIMDs, so its time hardly depends on the batch.
Medians over --reps calls after two warm-up calls; prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); extra = fn(); out.append(((time.perf_counter() - t0) * 1e3, extra))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = ge.load_package()
    lib = pkg._abi.bind_episode(pkg.load_hip_library())
    phases = pkg.problems.wb_trot_problem()
    B = a.batch
    s = pkg.MultiPhaseDDP(phases, batch=B)
    x0 = pkg.problems.wb_ensemble_x0(B, 20241222)
    s.set_initial_condition(x0); s.solve(pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=4))
    opt_rt = pkg.mhpc_ddp_setting(); opt_rt.max_AL_iter, opt_rt.max_DDP_iter = opt_rt.max_AL_iter_runtime, opt_rt.max_DDP_iter_runtime
    xs = np.ascontiguousarray(s.field(0, "XBAR")[:, 0])
    res = dict(batch=B, reps=a.reps, kernel_source_hash=pkg.kernel_source_hash(), waves_per_walk_launch=(B + 15) // 16)
    solve = timed(lambda: s.solve(opt_rt) or s.solve_time_ms(), a.reps)
    res["solve_runtime_limits_wall_ms"] = statistics.median(t for t, _ in solve); res["solve_runtime_limits_device_ms"] = statistics.median(e for _, e in solve)
    for n_exec in (50, 100):
        e = s.episode(n_exec, a.reps + 2)
        e.reset(xs)
        sim = lib.hsddp_episode_sim(e.e); ms = ctypes.c_float()

        def tick():
            e.advance(); lib.hsddp_sim_get_kernel_time_ms(sim, ctypes.byref(ms)); return float(ms.value)
        s.lib.hsddp_reset_kernel_times(s.h)
        t = timed(tick, a.reps)
        adv, walk = statistics.median(x for x, _ in t), statistics.median(k for _, k in t)
        kt = s.kernel_times(64)
        per = lambda k: kt[k][0] / kt[k][1] if k in kt and kt[k][1] else 0.0      # mean device time per launch over the warm-up and timed calls
        tag = f"n_exec_{n_exec}"
        res[tag] = dict(impacts=e.status()[2], advance_wall_ms=adv, walk_kernel_ms=walk, commit_kernel_ms=per("k_episode_commit"),
                        impact_kernel_ms=per("k_episode_impact"), impact_launches=kt.get("k_episode_impact", (0.0, 0))[1])
        res[tag]["host_and_sync_ms"] = adv - walk - res[tag]["commit_kernel_ms"] - res[tag]["impact_kernel_ms"]
        e.close()

        def manual():
            sim2 = pkg.Simulation(s, 1, n_exec)
            sim2.run(np.ascontiguousarray(xs[:, None])); _, xf = sim2.rows(); s.set_initial_condition(np.ascontiguousarray(xf[:, 0])); sim2.close()
        res[tag]["manual_tick_wall_ms"] = statistics.median(x for x, _ in timed(manual, a.reps))
        s.set_initial_condition(x0)
    s.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
