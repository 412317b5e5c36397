#!/usr/bin/env python3
"""Schedule-candidate ensembles on the MI355X (include/hsddp_ensemble.h); prints one JSON line.

  tick        batch 1, S timing candidates of the whole-body trot (N = --total), a fixed work of --tick-iters DDP iterations per solve:
              wall time of the S solves one after another vs side by side (one host thread and one stream per candidate), over --ticks
              ticks after --warmup; select + export of the winner's first 8 knots.
  throughput  S x --batch problems: DDP iterations per second sequential vs concurrent, per-candidate iteration imbalance, and
              k_ens_pack (8 knots of all S x batch pairs into device memory): time and GB/s from the bytes the shapes imply.
  dist        the sharded path (launch.shard_candidates): every rank solves its (candidate, state) segments, one all-gather of the tagged
              result rows, select_rows on every rank, one all-gather of the winners' policies.  --gpus N starts N ranks through
              launch.maybe_spawn exactly like bench.py (HSDDP_FORCE_PROCESS_GROUP=1 runs the RCCL calls on one rank).

  python tools/ensemble_bench.py [--gpus 1] [--ticks 20] [--batch 1024] [--dist-only] [--dump out.npz]
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

N_STEPS = 8


def tick_option(pkg, iters):
    return pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=iters, cost_thresh=0.0)


def reset(ens, cands, x0):
    for s, ph in zip(ens.solvers, cands):
        for i, p in enumerate(ph):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
    ens.set_initial_condition(x0)


def leg_tick(pkg, args):
    cands = pkg.problems.wb_trot_timing_candidates(args.total)[:args.S]
    ens = pkg.ScheduleEnsemble(cands, 1, device=args.device)
    x0 = pkg.problems.wb_ensemble_x0(1, args.seed)
    opt = tick_option(pkg, args.tick_iters)
    times = {"sequential": [], "concurrent": []}
    sel, exp = [], []
    for t in range(args.warmup + args.ticks):
        for mode in ("sequential", "concurrent") if t % 2 == 0 else ("concurrent", "sequential"):      # alternating: drift hits both alike
            reset(ens, cands, x0)
            t0 = time.perf_counter(); ens.solve(opt, concurrent=mode == "concurrent"); dt = (time.perf_counter() - t0) * 1e3
            if t >= args.warmup:
                times[mode].append(dt)
        t0 = time.perf_counter(); w, _ = ens.select(opt); t1 = time.perf_counter()
        ens.export_mpc_commands([(int(w[0]), 0)], N_STEPS); t2 = time.perf_counter()
        if t >= args.warmup:
            sel.append((t1 - t0) * 1e3); exp.append((t2 - t1) * 1e3)
    iters = ens.rows()[:, 0, 4].tolist()
    st = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90)), "max_ms": float(np.max(v))}
    out = {"S": len(cands), "total_knots": args.total, "ddp_iters_per_candidate": iters, "ticks": args.ticks,
           "sequential": st(times["sequential"]), "concurrent": st(times["concurrent"]),
           "speedup_median": float(np.median(times["sequential"]) / np.median(times["concurrent"])),
           "select_ms_median": float(np.median(sel)), "export_ms_median": float(np.median(exp))}
    ens.close()
    return out


def leg_throughput(pkg, args):
    import torch
    cands = pkg.problems.wb_trot_timing_candidates(args.total)[:args.S]
    S, B = len(cands), args.batch
    free, _ = torch.cuda.mem_get_info(args.device)
    ens = pkg.ScheduleEnsemble(cands, B, device=args.device)
    x0 = pkg.problems.wb_ensemble_x0(B, args.seed)
    opt = tick_option(pkg, args.tick_iters)
    res = {"S": S, "batch": B, "free_bytes_before": int(free)}
    for mode in ("warmup", "sequential", "concurrent"):
        reset(ens, cands, x0)
        t0 = time.perf_counter(); ens.solve(opt, concurrent=mode != "sequential"); dt = time.perf_counter() - t0
        rows = ens.rows()
        it = rows[:, :, 4].sum()
        if mode != "warmup":
            res[mode] = {"wall_s": dt, "ddp_iterations": int(it), "ddp_it_per_s": float(it / dt),
                         "per_candidate_solve_ms": [s.solve_time_ms() for s in ens.solvers]}
    per = rows[:, :, 4].sum(axis=1)
    res["per_candidate_iterations"] = per.astype(int).tolist()
    res["iteration_imbalance_max_over_mean"] = float(per.max() / per.mean())
    res["concurrent_over_sequential_it_per_s"] = res["concurrent"]["ddp_it_per_s"] / res["sequential"]["ddp_it_per_s"]
    # k_ens_pack: every (candidate, state) pair, 8 knots, into device memory
    pairs = np.array([(c, b) for c in range(S) for b in range(B)], dtype=np.int32)
    W = pkg.ensemble.command_row_words(N_STEPS)
    out = torch.empty((len(pairs), W), dtype=torch.int32, device=f"cuda:{args.device}")
    ts = []
    for r in range(6):
        t0 = time.perf_counter(); ens.export_mpc_commands(pairs, N_STEPS, out=out); ts.append(time.perf_counter() - t0)
    t = float(np.median(ts[1:]))
    wbytes = out.numel() * 4
    rbytes = len(pairs) * N_STEPS * (12 + 36 + 12 + 432 + 12 + 144 + 432) * 8 + len(pairs) * N_STEPS * 4 * 4      # fp64 fields + contacts
    res["pack"] = {"rows": len(pairs), "n_steps": N_STEPS, "write_bytes": wbytes, "read_bytes": rbytes, "call_ms_median": t * 1e3,
                   "GBps": (wbytes + rbytes) / t / 1e9, "fraction_of_6290GBps": (wbytes + rbytes) / t / 6.29e12,
                   "_note": "wall time of the whole call (pair upload, launch, synchronise): a lower bound of the kernel's own rate"}
    ens.close()
    return res


def leg_dist(pkg, args, rank, world, dist, device):
    launch = pkg.launch
    import torch
    cands = pkg.problems.wb_trot_timing_candidates(args.total)[:args.S]
    S, B = len(cands), args.dist_batch
    segs = launch.shard_candidates(S, B, world, rank)
    ens = pkg.ScheduleEnsemble([cands[c] for c, _, _ in segs], [n for _, _, n in segs], device=args.device)
    ens.set_initial_condition([pkg.problems.wb_ensemble_x0(n, args.seed, first=s) for _, s, n in segs])
    opt = tick_option(pkg, args.tick_iters)
    t0 = time.perf_counter(); ens.solve(opt, concurrent=True); solve_ms = (time.perf_counter() - t0) * 1e3
    rows = np.concatenate([pkg.ensemble.info_rows(s.get_info()) for s in ens.solvers])
    t0 = time.perf_counter()
    gathered = launch.gather_results(dist, launch.tagged_rows(segs, rows), device)
    g1 = (time.perf_counter() - t0) * 1e3
    all_rows = launch.ensemble_rows(gathered, S, B)
    winner = pkg.select_rows(all_rows, opt)
    W = pkg.ensemble.command_row_words(N_STEPS)

    def pack(pairs):
        out = torch.empty((len(pairs), W), dtype=torch.int32, device=device)
        return ens.export_mpc_commands(pairs, N_STEPS, out=out) if pairs else out
    t0 = time.perf_counter()
    policies = launch.gather_policies(dist, S, B, winner, pack, W, device)
    g2 = (time.perf_counter() - t0) * 1e3
    per_rank = launch.gather_scalars(dist, [solve_ms, g1, g2, float(rows[:, 4].sum())], device)
    ens.close()
    return {"S": S, "batch": B, "world": world, "per_rank": {"solve_ms": per_rank[:, 0].tolist(), "rows_gather_ms": per_rank[:, 1].tolist(),
            "policy_gather_ms": per_rank[:, 2].tolist(), "ddp_iterations": per_rank[:, 3].tolist()},
            "winners": np.bincount(winner, minlength=S).tolist()}, winner, policies, all_rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--S", type=int, default=4)
    ap.add_argument("--total", type=int, default=200)
    ap.add_argument("--tick-iters", type=int, default=4)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dist-batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=20241220)
    ap.add_argument("--dist-only", action="store_true")
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--dump", default=None, help="npz with the dist leg's gathered winners, policies and rows")
    args = ap.parse_args()
    pkg = ge.load_package()
    launch = pkg.launch
    rc = launch.maybe_spawn(args.gpus, os.path.abspath(__file__), sys.argv[1:])      # before anything touches the GPU
    if rc is not None:
        sys.exit(rc)
    rank, world, local, dist = launch.init_ranks("nccl")
    args.device = local
    import torch
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    line = {"metric": "schedule_ensemble", "n_gpus": world, "collectives": "rccl" if dist is not None else "none",
            "kernel_source_hash": pkg.kernel_source_hash()}
    if world == 1 and not args.dist_only:
        line["tick"] = leg_tick(pkg, args)
        if not args.no_throughput:
            line["throughput"] = leg_throughput(pkg, args)
    line["dist"], winner, policies, rows = leg_dist(pkg, args, rank, world, dist, device)
    if rank == 0:
        if args.dump:
            np.savez(args.dump, winner=winner, policies=policies, rows=rows)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier(); dist.destroy_process_group()


if __name__ == "__main__":
    main()
