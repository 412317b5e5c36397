#!/usr/bin/env python3
"""Per-sample plant (include/hsddp_plant.h; the _plant kernels of csrc/hsddp_plant.hip): what reading the row and the always-on records and sub-step loop
cost beside the twin kernel without the plant, per family; one JSON line.

  The shape of tools/terrain_bench.py: config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve,
  --samples 16 perturbed initial states per problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) resident on the device, the whole --window (200 steps),
  force records on (mu 0.6, fz_min 0), S = --substeps (2), hsddp_sim_run.  Families:
    bi    the bilateral walk (off: k_sim_quad_grf_sub)
    uni   unilateral contact with --fz-rel (0) on the plane z = 0 (off: k_sim_quad_uni)
    ter   that with a flat terrain and early touchdown, w_td 0.05 (off: k_sim_quad_ter)
  and per family three variants:
    <f>_off       the plant off: the parent commit's kernels
    <f>_nominal   a one-row nominal table: the _plant kernel doing the same arithmetic
    <f>_varied    a 256-row table - payloads of 0 .. 2 kg within 8 cm of the trunk origin, link scales 0.8 .. 1.2, gains 0.85 .. 1.1, friction 0 .. 0.01 -
                  with a row drawn per sample
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel time (HIP
  events around the launch), median and min / max over the rounds; for the two plant variants the ratio to <f>_off, median and min / max of the per-round
  ratios.  The last round is summarised: diverged samples, min_height, max_torque.

  The off rows of ANOTHER build of the library - the parent commit's - are measured by the same tool: HSDDP_HIP_VARIANT=<name> python tools/plant_bench.py
  --only-parent, alternated with runs of this build by the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/plant_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--substeps 2] [--fz-rel 0] [--only-parent] [--timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def varied_table(pkg, np, n_rows, shape, seed=20241222):
    rng = np.random.default_rng(seed)
    sm = pkg.sim
    nom = sm.Plant.nominal().rows[0]
    rows = []
    for _ in range(n_rows):
        r = sm.with_trunk(nom, *sm.payload_trunk(rng.uniform(0.0, 2.0), rng.uniform(-0.08, 0.08, 3)))
        r = sm.with_damping(sm.with_gain(sm.with_link_scale(r, rng.uniform(0.8, 1.2, 12)), rng.uniform(0.85, 1.1, 12)), rng.uniform(0.0, 0.01, 12))
        rows.append(r)
    return sm.Plant(np.stack(rows), plant_of=rng.integers(0, n_rows, size=shape).astype(np.int32))


def child(args):
    import numpy as np
    import torch
    dev = f"cuda:{args.device}"
    torch.zeros(1, device=dev)      # torch's HIP runtime up before the package's library is loaded
    import __graft_entry__ as ge
    pkg = ge.load_package()
    phases = pkg.problems.wb_trot_problem()
    B, R, n = args.batch, args.samples, args.window
    s = pkg.MultiPhaseDDP(phases, batch=B, device=args.device)
    s.set_initial_condition(pkg.problems.wb_ensemble_x0(B, 20241220))
    s.solve(pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=args.steps, cost_thresh=0.0))
    xb0 = s.field(0, "XBAR")[:, 0]
    d = pkg.problems.perturbed_states(np.zeros((1, 36)), R, 0.02, 0.2, seed=20241222)[0]      # one set of R perturbations for every problem
    xs = torch.from_numpy(np.ascontiguousarray(xb0[:, None, :] + d[None])).to(dev)
    sim = pkg.Simulation(s, R, n)
    sim.set_grf(0.6); sim.set_substeps(args.substeps)
    kinds = ["off"] if args.only_parent else ["off", "nominal", "varied"]
    variants = [(f"{f}_{k}", f, k) for f in ("bi", "uni", "ter") for k in kinds]
    plants = {} if args.only_parent else {"nominal": pkg.sim.Plant.nominal(), "varied": varied_table(pkg, np, 256, (B, R))}
    flat = pkg.sim.Terrain(H=np.zeros((1, 1, 1)), early=True, w_td=0.05)

    def run(name, family, kind):
        if family == "bi":
            sim.clear_contact()
        else:
            sim.set_contact(args.fz_rel, 0.0)
        if family == "ter":
            sim.set_terrain(flat)
        else:
            sim.clear_terrain()
        if not args.only_parent:
            if kind in plants:
                sim.set_plant(plants[kind])
            else:
                sim.clear_plant()
        sim.run(xs)
        return sim.kernel_time_ms()
    for v in variants:      # warm-up: code objects loaded, every buffer allocated
        run(*v)
    k_ms = {v[0]: [] for v in variants}; stats = {}
    for rnd in range(args.runs):
        for v in variants:
            k_ms[v[0]].append(run(*v))
            if rnd == args.runs - 1:
                rows, xf = sim.rows()
                ok = rows["first_bad"] < 0
                stats[v[0]] = {"diverged_samples": int((~ok).sum()), "min_height_live": float(rows["min_height"][ok].min()), "median_min_height": float(np.median(rows["min_height"])),
                               "median_max_torque": float(np.median(rows["max_torque"]))}
    sim.close()
    variant = bool(os.environ.get("HSDDP_HIP_VARIANT", ""))
    res = {"metric": "plant", "kernel_source_hash": None if variant else pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B, "samples": R,
           "window": n, "substeps": args.substeps, "solve_steps": args.steps, "runs": args.runs, "fz_rel": args.fz_rel, "variants": {}}
    for name, family, kind in variants:
        a = np.array(k_ms[name])
        res["variants"][name] = {"kernel_ms": k_ms[name], "median_kernel_ms": float(np.median(a)), "min_kernel_ms": float(a.min()), "max_kernel_ms": float(a.max()),
                                 "sample_knots_per_s_kernel": B * R * n / (float(np.median(a)) * 1e-3), **stats[name]}
        if kind != "off":
            q = a / np.array(k_ms[f"{family}_off"])
            res["variants"][name].update(kernel_over_off=float(np.median(a) / np.median(k_ms[f"{family}_off"])), round_ratio_median=float(np.median(q)), round_ratio_min=float(q.min()),
                                         round_ratio_max=float(q.max()))
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--substeps", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fz-rel", type=float, default=0.0)
    ap.add_argument("--only-parent", action="store_true", help="the rows with the plant off alone, through the entry points the parent commit's library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"plant_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
