#!/usr/bin/env python3
"""Terrain height maps and early swing-foot touchdown (include/hsddp_terrain.h; k_sim_quad_ter): what the lookup and the wider tested set cost beside
the run with unilateral contact alone, and what they do to the statistics of a run; one JSON line.

  The shape of tools/contact_bench.py: config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve,
  --samples 16 perturbed initial states per problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) resident on the device, the whole --window (200
  steps), force records on (mu 0.6, fz_min 0), unilateral contact with --fz-rel (0) on the plane z = 0, hsddp_sim_run.  Variants, each at S = 1 and 4:
    off_s1 / off_s4        the contact rule off (k_sim_quad_grf / k_sim_quad_grf_sub)
    uni_s1 / uni_s4        (a) contact on, terrain off (k_sim_quad_uni)
    flat_s1 / flat_s4      (b) terrain on, H = 0, early = 0: the cost of the lookup and of carrying E
    early_s1 / early_s4    (c) as (b) with early = 1, w_td = --w-td (0.05): the swing feet are tested too - what the fleet does on flat ground
    rough_s1 / rough_s4    (d) 64 seeded maps of 64 x 64 cells of 5 cm, heights N(0, 1 cm), a map drawn per sample, early = 1
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel time
  (HIP events around the launch), median and min / max over the rounds; for (b) - (d) the ratio to (a) of the same S, median and min / max of the
  per-round ratios.  The last round is summarised: diverged samples, min_height, the contact rows, the terrain rows, and - from one further untimed
  hsddp_mc_run with fall_height 0.16 alone - the fallen samples.

  The off and (a) rows of ANOTHER build of the library - the parent commit's - are measured by the same tool: HSDDP_HIP_VARIANT=<name> python
  tools/terrain_bench.py --only-parent (a library without the terrain entry points has nothing else to measure), alternated with runs of this build
  by the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/terrain_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--fz-rel 0] [--w-td 0.05] [--only-parent] [--timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys

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
    d = pkg.problems.perturbed_states(np.zeros((1, 36)), R, 0.02, 0.2, seed=20241222)[0]      # one set of R perturbations for every problem
    xs = torch.from_numpy(np.ascontiguousarray(xb0[:, None, :] + d[None])).to(dev)
    sim = pkg.Simulation(s, R, n)
    sim.set_grf(0.6)
    kinds = ["off", "uni"] if args.only_parent else ["off", "uni", "flat", "early", "rough"]
    variants = [(f"{k}_s{S}", S, k) for S in (1, 4) for k in kinds]
    terrains = {}
    if not args.only_parent:
        T = pkg.sim.Terrain
        rng = np.random.default_rng(20241222)
        terrains["flat"] = T(H=np.zeros((1, 1, 1)), early=False)
        terrains["early"] = T(H=np.zeros((1, 1, 1)), early=True, w_td=args.w_td)
        terrains["rough"] = T(H=0.01 * rng.standard_normal((64, 64, 64)), x0=-1.1, y0=-1.6, cx=0.05, cy=0.05, early=True, w_td=args.w_td,
                              map_of=rng.integers(0, 64, size=(B, R)).astype(np.int32))

    def run(name, S, kind):
        sim.set_substeps(S)
        if kind == "off":
            sim.clear_contact()
        else:
            sim.set_contact(args.fz_rel, 0.0)
        if not args.only_parent:
            if kind in terrains:
                sim.set_terrain(terrains[kind])
            else:
                sim.clear_terrain()
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
                st = {"diverged_samples": int((~ok).sum()), "min_height_live": float(rows["min_height"][ok].min()), "median_min_height": float(np.median(rows["min_height"]))}
                if v[2] != "off":
                    c = sim.contact_rows()
                    st.update(releasing_samples=int((c["n_release"] > 0).sum()), n_release=int(c["n_release"].sum()), n_land=int(c["n_land"].sum()), n_free=int(c["n_free"].sum()),
                              max_lift=float(c["max_lift"].max()))
                if v[2] in terrains:
                    t = sim.terrain_rows()
                    fe = t["first_early"][t["first_early"] >= 0]
                    st.update(early_samples=int((t["n_early"] > 0).sum()), n_early=int(t["n_early"].sum()), n_early_release=int(t["n_early_release"].sum()), n_held=int(t["n_held"].sum()),
                              held_at_end_samples=int((t["early_final"] != 0).sum()), median_first_early=float(np.median(fe)) if fe.size else None, max_pen=float(t["max_pen"].max()),
                              early_per_live_sample=float(t["n_early"][ok].mean()) if ok.any() else None)
                sim.run(xs, dist=Dist(seed=20241222, fall_height=0.16))      # untimed: the fall statistic of the same run
                e = sim.extra()
                ff = e["first_fall"][e["first_fall"] >= 0]
                st.update(fallen_samples=int(ff.size), median_first_fall=float(np.median(ff)) if ff.size else None)
                stats[v[0]] = st
    sim.close()
    variant = bool(os.environ.get("HSDDP_HIP_VARIANT", ""))
    res = {"metric": "terrain", "kernel_source_hash": None if variant else pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B, "samples": R,
           "window": n, "solve_steps": args.steps, "runs": args.runs, "fz_rel": args.fz_rel, "w_td": args.w_td, "variants": {}}
    for name, S, kind in variants:
        a = np.array(k_ms[name])
        res["variants"][name] = {"substeps": S, "kernel_ms": k_ms[name], "median_kernel_ms": float(np.median(a)), "min_kernel_ms": float(a.min()), "max_kernel_ms": float(a.max()),
                                 "sample_knots_per_s_kernel": B * R * n / (float(np.median(a)) * 1e-3), **stats[name]}
        if kind in terrains:
            q = a / np.array(k_ms[f"uni_s{S}"])
            res["variants"][name].update(kernel_over_uni=float(np.median(a) / np.median(k_ms[f"uni_s{S}"])), round_ratio_median=float(np.median(q)), round_ratio_min=float(q.min()),
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
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fz-rel", type=float, default=0.0)
    ap.add_argument("--w-td", type=float, default=0.05)
    ap.add_argument("--only-parent", action="store_true", help="the rows without the terrain alone, through the entry points the parent commit's library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"terrain_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
