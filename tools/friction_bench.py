#!/usr/bin/env python3
"""Coulomb friction (include/hsddp_friction.h; k_sim_quad_fric): what carrying the rule costs beside the run with the contact rule alone, and what a floor
that lets feet slide does to the statistics of a run; one JSON line.

  Config 3 handle (problems.wb_trot_problem(), WB N = 200, --batch 4096) after a --steps iteration solve, --samples 16 perturbed initial states per
  problem (sigma_q 0.02, sigma_v 0.2 around Xbar[0]) resident on the device, the whole --window (200 steps), force records on (mu 0.6, fz_min 0), the
  contact rule on (fz_rel = --fz-rel, z_ground = 0), hsddp_sim_run.  Variants, each at S = 1 and S = 4:
    off_s1 / off_s4          (a) friction off: k_sim_quad_uni, the kernels of the parent commit
    carry_s1 / carry_s4      (b) friction on with mu_s = mu_k = 1e9: the cost of carrying the rule
    mu06_s1 / mu06_s4        (c) friction on at mu_s = mu_k = 0.6
    mu03_s1 / mu03_s4        (d) friction on at mu_s = mu_k = 0.3
  --runs rounds; in every round each variant runs once, in the order above, so the variants are ALTERNATED in one session.  Per variant: kernel
  time (HIP events around the launch), medians and min / max over the rounds; for (b) - (d) the ratio to (a) of the same S.  The last round is
  summarised: diverged samples, first_bad, min_height, the samples that left the pyramid (records' mu 0.6: over sticking feet only once friction is
  on), the friction rows - samples that slide, onsets, re-sticks, mean slide distance of the sliding samples, largest speed - and, from one further
  untimed hsddp_mc_run with fall_height 0.16 alone, first_fall.

  The (a) rows of ANOTHER build of the library - the parent commit's - are measured by the same tool: HSDDP_HIP_VARIANT=<name> python
  tools/friction_bench.py --only-off (a library without the friction entry points has nothing else to measure), alternated with runs of this build
  by the caller.

The measurement runs in a child process under --timeout seconds; a child that fails or runs out of time ends the tool with its status.

  python tools/friction_bench.py [--batch 4096] [--samples 16] [--steps 10] [--runs 10] [--window 200] [--fz-rel 0.0] [--v-stick 0.02] [--only-off] [--timeout 600]
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
    sim.set_contact(args.fz_rel, 0.0)
    # (name, S, rule: None friction off / mu_s = mu_k)
    variants = [("off_s1", 1, None), ("off_s4", 4, None)]
    if not args.only_off:
        variants = [("off_s1", 1, None), ("carry_s1", 1, 1e9), ("mu06_s1", 1, 0.6), ("mu03_s1", 1, 0.3), ("off_s4", 4, None), ("carry_s4", 4, 1e9), ("mu06_s4", 4, 0.6), ("mu03_s4", 4, 0.3)]

    def setup(name, S, rule):
        sim.set_substeps(S)
        if not args.only_off:
            if rule is None:
                sim.clear_friction()
            else:
                sim.set_friction(pkg.sim.Friction(mu=[[rule, rule]], v_stick=args.v_stick))

    def run(name, S, rule):
        setup(name, S, rule)
        sim.run(xs)
        return sim.kernel_time_ms()
    for v in variants:      # warm-up: code objects loaded, every buffer allocated
        run(*v)
    k_ms = {v[0]: [] for v in variants}; stats = {}
    for rnd in range(args.runs):
        for v in variants:
            k_ms[v[0]].append(run(*v))
            if rnd == args.runs - 1:
                rows, xf = sim.rows(); g = sim.grf()
                ok = rows["first_bad"] < 0
                fb = rows["first_bad"][~ok]
                st = {"diverged_samples": int((~ok).sum()), "median_first_bad": float(np.median(fb)) if fb.size else None, "first_first_bad": int(fb.min()) if fb.size else None,
                      "min_height_live": float(rows["min_height"][ok].min()), "median_min_height": float(np.median(rows["min_height"])),
                      "slipping_samples": int((g["first_slip"] >= 0).sum()), "pulling_samples": int((g["min_fz"] < 0).sum()), "n_slip": int(g["n_slip"].sum()),
                      "min_fz": float(g["min_fz"].min())}
                c = sim.contact_rows()
                if v[2] is not None:
                    f = sim.friction_rows()
                    sl = f["n_onset"] > 0
                    st.update(sliding_samples=int(sl.sum()), n_onset=int(f["n_onset"].sum()), n_restick=int(f["n_restick"].sum()), n_slide=int(f["n_slide"].sum()),
                              sliding_at_end_samples=int((f["slide_final"] != 0).sum()), mean_distance_sliding=float(f["distance"][sl].mean()) if sl.any() else 0.0,
                              max_speed=float(f["max_speed"].max()), median_first_slide=float(np.median(f["first_slide"][sl])) if sl.any() else None)
                st.update(releasing_samples=int((c["n_release"] > 0).sum()), n_release=int(c["n_release"].sum()), n_land=int(c["n_land"].sum()), n_free=int(c["n_free"].sum()),
                          free_at_end_samples=int((c["free_final"] != 0).sum()), max_lift=float(c["max_lift"].max()))
                sim.run(xs, dist=Dist(seed=20241222, fall_height=0.16))      # untimed: the fall statistic of the same run
                e = sim.extra()
                ff = e["first_fall"][e["first_fall"] >= 0]
                st.update(fallen_samples=int(ff.size), median_first_fall=float(np.median(ff)) if ff.size else None)
                stats[v[0]] = st
    sim.close()
    variant = bool(os.environ.get("HSDDP_HIP_VARIANT", ""))
    res = {"metric": "coulomb_friction", "fz_rel": args.fz_rel, "v_stick": args.v_stick, "kernel_source_hash": None if variant else pkg.kernel_source_hash(), "library": os.path.basename(pkg.HIP_LIB_PATH), "batch": B, "samples": R,
           "window": n, "solve_steps": args.steps, "runs": args.runs, "variants": {}}
    med = {name: float(np.median(k_ms[name])) for name, _, _ in variants}
    for name, S, rule in variants:
        res["variants"][name] = {"substeps": S, "mu": rule, "kernel_ms": k_ms[name], "median_kernel_ms": med[name], "min_kernel_ms": float(min(k_ms[name])),
                                 "max_kernel_ms": float(max(k_ms[name])), "sample_knots_per_s_kernel": B * R * n / (med[name] * 1e-3), **stats[name]}
        if rule is not None:
            res["variants"][name]["kernel_over_off"] = med[name] / med[f"off_s{S}"]
        if name.startswith("mu0"):
            res["variants"][name]["kernel_over_carry"] = med[name] / med[f"carry_s{S}"]
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
    ap.add_argument("--fz-rel", type=float, default=0.0, help="release threshold of the contact rule, on in every variant")
    ap.add_argument("--v-stick", type=float, default=0.02)
    ap.add_argument("--only-off", action="store_true", help="the rows with friction off alone, through the entry points every build of the library has")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the tool starts under its time limit)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        return subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(f"friction_bench: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
