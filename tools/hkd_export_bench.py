#!/usr/bin/env python3
"""HKD-MPC command export at the config-5 shape (include/hsddp_hkd.h); prints one JSON line.

problems.hkd_bound_problem() (N = 200), an fp32 handle of --batch problems (16 384: config 5) after a short solve, --n-steps knots per message:
  batched  hsddp_export_hkd_commands of the whole batch into device memory, status times and pf_in passed: median wall time
           per call (the call returns after its stream has finished), algorithmic bytes from the shapes, GB/s.
  batch-1  hsddp_export_hkd_command of one problem into host memory: median latency.
Kernel time: run this under `rocprofv3 --kernel-trace --stats -- python tools/hkd_export_bench.py` and read k_pack_hkd there.

  python tools/hkd_export_bench.py [--batch 16384] [--n-steps 9] [--calls 50]
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

HBM_PEAK_TBS = 8.0      # MI355X HBM3E, theoretical


def algorithmic_bytes(nb, n_steps):
    """Writes: one 7 816-byte row per problem.  Reads per problem: n_steps x (Ubar 24 + Xbar 12 + K block 144) doubles, 4 footholds x 3 doubles,
    pf_in 12 floats."""
    rd = nb * (n_steps * (24 + 12 + 144) * 8 + 96 + 48)
    wr = nb * 1954 * 4
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--n-steps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    pkg = ge.load_package()
    import ctypes
    rt = ctypes.CDLL("libamdhip64.so.7")      # the HIP runtime libhsddp_hip.so runs on: the device destination
    phases = pkg.problems.hkd_bound_problem()
    x0 = pkg.problems.hkd_ensemble_x0(args.batch, 20241220, phases)
    s = pkg.MultiPhaseDDP(phases, batch=args.batch, device=args.device, precision=pkg.PREC_F32)
    s.set_initial_condition(x0)
    t0 = time.perf_counter(); s.solve(pkg.problems.hkd_ddp_setting(max_AL_iter=1, max_DDP_iter=2)); solve_ms = (time.perf_counter() - t0) * 1e3
    st = np.tile(np.array([0.16, 0.16, 0.06, 0.06]), (len(phases), 1))
    pf = np.random.default_rng(1).standard_normal((args.batch, 12)).astype(np.float32)
    p = ctypes.c_void_p()
    if rt.hipMalloc(ctypes.byref(p), ctypes.c_size_t(args.batch * 1954 * 4)) != 0:
        raise RuntimeError("hipMalloc of the destination failed")
    kw = dict(n_steps=args.n_steps, mpc_time=0.0, dt=0.01, status_times=st, pf=pf)
    times = []
    for c in range(args.warmup + args.calls):
        t0 = time.perf_counter(); s.export_hkd_commands(0, args.batch, out=p.value, **kw); dt = time.perf_counter() - t0
        if c >= args.warmup:
            times.append(dt)
    lat = []
    for c in range(args.warmup + 4 * args.calls):
        t0 = time.perf_counter(); s.export_hkd_command(c % args.batch, args.n_steps, 0.0, 0.01, st, pf[c % args.batch]); dt = time.perf_counter() - t0
        if c >= args.warmup:
            lat.append(dt)
    # the device rows against the host-destination call (same launch, staged copy): a cheap sanity check of the measured path
    host = s.export_hkd_commands(0, 64, **{**kw, "pf": pf[:64]})
    dev = np.zeros_like(host)
    ok = rt.hipMemcpy(ctypes.c_void_p(dev.ctypes.data), p, ctypes.c_size_t(dev.nbytes), 2) == 0 and bool(np.array_equal(dev, host))      # device to host
    rt.hipFree(p)
    rd, wr = algorithmic_bytes(args.batch, args.n_steps)
    med = float(np.median(times))
    res = {"metric": "hkd_export", "batch": args.batch, "n_steps": args.n_steps, "precision": "fp32", "knots": sum(p["desc"].horizon for p in phases),
           "solve_ms": solve_ms, "calls": args.calls,
           "batched_median_ms": med * 1e3, "batched_min_ms": float(np.min(times)) * 1e3, "batched_p90_ms": float(np.percentile(times, 90)) * 1e3,
           "algorithmic_read_bytes": rd, "algorithmic_write_bytes": wr, "algorithmic_bytes": rd + wr,
           "gbps_by_wall_time": (rd + wr) / med / 1e9, "fraction_of_hbm_peak_by_wall_time": (rd + wr) / med / 1e12 / HBM_PEAK_TBS,
           "batch1_median_us": float(np.median(lat)) * 1e6, "batch1_p90_us": float(np.percentile(lat, 90)) * 1e6,
           "device_rows_equal_host_rows": ok, "kernel": "k_pack_hkd", "kernel_source_hash": pkg.kernel_source_hash()}
    print(json.dumps(res))
    s.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
