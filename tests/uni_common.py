"""Shared by tests/test_contact_host.py and tests/test_contact_gpu.py: the reference of a closed-loop window with UNILATERAL GROUND CONTACT
(include/hsddp_contact.h), the host build of the program (tests/_emu/uni_emu.cpp) behind numpy arguments, and the comparison against the reference.

Reference: walk_ref.reference_walk with the contact rule on - the four rules of the header, in numpy on the oracle's existing probes only.  The walk
takes an initial F (episode ticks) and returns the forces and attached sets of every substep's LAST solve, the contact rows and, per sample, the MARGIN
of its decisions.

Tolerances.  X, U, x_final, the summaries, the forces and max_lift: sim_common.compare_window / grf_common.force_bound, 1e-8 x scale.  The integers
and free_final EXACTLY, but for a sample whose reference comes within grf_common.MARGIN_FACTOR x the bound of a decision; at most ONE such sample per
case is left out (its floats are left out with it: behind a flipped decision the trajectories differ).  A decision and its margin:
  - a solve keeps or releases its feet: |lambda_z - fz_rel| of every attached foot of every solve, against the force bound;
  - which foot is released: the gap between the two smallest lambda_z, against the force bound;
  - a landing test (p_z <= z_ground and w_z < 0): true - the smaller of |p_z - z_ground| and |w_z|; false - the larger over the conditions that
    fail; against the trajectory bound 1e-8 (metres, metres per second).
The amplification of a 1e-12 change of x0 through the event-carrying windows is measured by test_contact_host.py and printed."""
import numpy as np

import sim_common as sc
import mc_common as mc
import grf_common as gc
import walk_ref as wr

TRAJ_BOUND = sc.RTOL      # positions and velocities of order one


def oracle_walk_uni(pkg, oracle_lib, phases, policy, smap, x0, S, fz_rel, z_ground, dist=None, kick=None, F0=None):
    """x0: [B, R, 36]; F0: None or bool [B, R, 4].  Returns what sub_common.oracle_walk_sub returns - Y [B, R, n, S, 12] of the LAST solve of every
    substep - and att [B, R, n, S, 4] (the set that solve ran on), rows (CONTACT_ROW_DTYPE [B, R]), F [B, R, 4] at the end, solves [B, R] (contact
    solves made), force_margin and kin_margin [B, R] (see the head of the file), raw_kin (smallest |p_z - z_ground|, |w_z| over all tests)."""
    w = wr.reference_walk(pkg, oracle_lib, phases, policy, smap, x0, S, contact=(fz_rel, z_ground), dist=dist, kick=kick, F0=F0)
    return wr.pick(w, wr.KEYS_UNI)


def grf_rows_uni(pkg, ref, mu, fz_min):
    """The force records of a run with the rule on: sim.grf_rows_sub's statement over the ATTACHED (foot, substep) pairs that count."""
    Y = ref["Y"]
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    st = ref["att"] & ref["counted"][..., None]
    fz = F[..., 2]
    cone = mu * fz - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    viol = st & ((fz < fz_min) | (cone < 0.0))
    out = np.zeros(Y.shape[:-3], dtype=pkg._abi.GRF_ROW_DTYPE)
    out["min_fz"] = np.where(st, fz, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["min_cone"] = np.where(st, cone, np.inf).min(axis=(-3, -2, -1), initial=np.inf)
    out["max_fz"] = np.where(st, fz, -np.inf).max(axis=(-3, -2, -1), initial=-np.inf)
    step = viol.any(axis=(-2, -1))
    out["first_slip"] = np.where(step.any(axis=-1), step.argmax(axis=-1), -1)
    out["n_slip"] = viol.sum(axis=(-3, -2, -1))
    rec_margin = np.minimum(np.where(st, np.abs(cone), np.inf).min(axis=(-3, -2, -1), initial=np.inf), np.where(st, np.abs(fz - fz_min), np.inf).min(axis=(-3, -2, -1), initial=np.inf))
    return out, rec_margin


def near_samples(tag, ref, rec_margin=None):
    """The samples of the reference within MARGIN_FACTOR x the bound of a decision; asserts that there is at most one (on the REFERENCE alone)."""
    fb = gc.force_bound(ref["Y"])
    near = (ref["force_margin"] < gc.MARGIN_FACTOR * fb) | (ref["kin_margin"] < gc.MARGIN_FACTOR * TRAJ_BOUND)
    if rec_margin is not None:
        near = near | (rec_margin < gc.MARGIN_FACTOR * fb)
    if "sat_margin" in ref:
        near = near | (ref["sat_margin"] < mc.NEAR) | (ref["fall_margin"] < mc.NEAR)
    r = ref["rows"]
    print(f"[uni] {tag}: force bound {fb:.3e} N (needed margin {gc.MARGIN_FACTOR * fb:.3e}), smallest force margin {ref['force_margin'].min():.3e} N, smallest landing "
          f"margin {ref['kin_margin'].min():.3e} (needed {gc.MARGIN_FACTOR * TRAJ_BOUND:.1e}; raw |p_z - z_g| {ref['raw_kin'][0]:.3e}, |w_z| {ref['raw_kin'][1]:.3e}), "
          f"releases {int(r['n_release'].sum())} on {int((r['n_release'] > 0).sum())} samples, landings {int(r['n_land'].sum())}, free pairs {int(r['n_free'].sum())}, "
          f"solves per sample {ref['solves'].min()} .. {ref['solves'].max()}, left out {int(near.sum())} (force {int((ref['force_margin'] < gc.MARGIN_FACTOR * fb).sum())}, "
          f"landing {int((ref['kin_margin'] < gc.MARGIN_FACTOR * TRAJ_BOUND).sum())}, records {0 if rec_margin is None else int((rec_margin < gc.MARGIN_FACTOR * fb).sum())})")
    assert near.sum() <= 1, f"{tag}: {int(near.sum())} samples of the reference lie within the margin of a decision"
    return near


def compare_case(tag, pkg, res, ref, xbar, mu=0.0, fz_min=0.0, fz_rel=None):
    """One run with the rule on against its reference walk.  res: rows, x_final, X, U, contact and, with records, grf and Y (and extra)."""
    want_g, rec_margin = grf_rows_uni(pkg, ref, mu, fz_min) if "grf" in res else (None, None)
    near = near_samples(tag, ref, rec_margin)
    keep = ~near
    cut = lambda a: np.asarray(a)[keep][None]      # the samples that are compared, as one "problem"
    xb = np.broadcast_to(xbar[:, None], ref["X"].shape)[keep]      # each kept sample with its own problem's Xbar
    sub = dict(rows=res["rows"][keep][None], x_final=cut(res["x_final"]))
    if "X" in res:
        sub["X"], sub["U"] = cut(res["X"]), cut(res["U"])
    # compare_window takes Xbar per problem: here every kept sample is a problem of its own
    flat = {k: (v[0][:, None] if k != "rows" else v[0][:, None]) for k, v in sub.items()}
    fb = ref["first_bad"][keep]
    live = fb < 0
    if live.all():
        sc.compare_window(tag, flat, ref["X"][keep][:, None], ref["U"][keep][:, None], xb)
    else:      # a case with a contained divergence: the window of the live samples, first_bad of all
        lv = {k: v[live] for k, v in flat.items()}
        sc.compare_window(tag, lv, ref["X"][keep][live][:, None], ref["U"][keep][live][:, None], xb[live])
    assert np.array_equal(res["rows"]["first_bad"][keep], fb), (tag, res["rows"]["first_bad"], ref["first_bad"])
    got, want = res["contact"], ref["rows"]
    for f in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(got[f][keep], want[f][keep]), (tag, f, got[f], want[f])
    sc.close(f"{tag} max_lift", got["max_lift"][keep], want["max_lift"][keep], scale=1.0)
    if "extra" in res:
        assert np.array_equal(res["extra"]["n_sat"][keep], ref["n_sat"][keep]) and np.array_equal(res["extra"]["first_fall"][keep], ref["first_fall"][keep]), tag
    if "grf" in res:
        bound = gc.force_bound(ref["Y"]); scale = bound / sc.RTOL
        if res.get("Y") is not None:
            sc.close(tag + " Y", res["Y"][keep], ref["Y"][keep][..., 0, :], scale=scale)
            free = ~np.repeat(ref["att"][keep][..., 0, :], 3, axis=-1)
            assert (res["Y"][keep][free] == 0.0).all(), f"{tag}: the force entry of a foot that is not attached is not exactly 0"
        for f in ("min_fz", "min_cone", "max_fz"):
            a, w = res["grf"][f][keep], want_g[f][keep]
            assert np.array_equal(np.isfinite(a), np.isfinite(w)) and np.array_equal(a[~np.isfinite(w)], w[~np.isfinite(w)]), (tag, f)
            sc.close(f"{tag} {f}", a[np.isfinite(w)], w[np.isfinite(w)], scale=scale)
        assert np.array_equal(res["grf"]["first_slip"][keep], want_g["first_slip"][keep]), (tag, res["grf"]["first_slip"], want_g["first_slip"])
        assert np.array_equal(res["grf"]["n_slip"][keep], want_g["n_slip"][keep]), (tag, res["grf"]["n_slip"], want_g["n_slip"])
        if fz_rel is not None:
            fin = np.isfinite(res["grf"]["min_fz"])
            assert (res["grf"]["min_fz"][fin] >= fz_rel - bound).all(), tag
    return near


def invariants(tag, res, fz_rel, bound):
    """Properties of a run's own outputs (no reference): an attached foot's Y_z >= fz_rel - bound and a free or swing foot's force exactly 0 cannot be
    told apart from Y alone, so: every nonzero Y_z is >= fz_rel - bound; min_fz >= fz_rel - bound where finite; n_free = 0 <=> n_release = 0 for a run
    that starts with F empty."""
    Yz = res["Y"].reshape(res["Y"].shape[:-1] + (4, 3))
    nz = (Yz != 0.0).any(axis=-1)
    assert (Yz[..., 2][nz] >= fz_rel - bound).all(), tag
    fin = np.isfinite(res["grf"]["min_fz"])
    assert fin.any() and (res["grf"]["min_fz"][fin] >= fz_rel - bound).all(), tag
    c = res["contact"]
    assert np.array_equal(c["n_free"] == 0, c["n_release"] == 0), (tag, c["n_free"], c["n_release"])


# ---- the host build of the program

def build_emu(tmpdir):
    lib = wr.build_so(tmpdir, "uni_emu.cpp", "libhsddp_uni_emu.so")
    assert [lib.uni_emu_park_doubles(m) for m in (0, 1)] == [39, 41]      # the parked column of the three kernels, doubles per lane
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, fz_rel, z_ground, dist=None, kick=None, mu=0.0, fz_min=0.0, F=None, hold=None):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; F: None or float [R, 4], updated in place.  Returns raw arrays."""
    args, out, keep = wr.emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min)
    tail, out["c"] = wr.emu_contact_args(x0.shape[0], fz_rel, z_ground, F, hold)
    assert lib.uni_emu_run(*args, *tail) == 0
    return out


def contact_rows_of(pkg, raw):
    return wr.struct_rows(raw, pkg._abi.CONTACT_ROW_DTYPE)


def emu_result(pkg, outs, disturbed, records):
    import sub_common as sub
    res = sub.emu_result(pkg, outs, disturbed, records)
    res["contact"] = contact_rows_of(pkg, np.stack([o["c"] for o in outs]))
    return res


def host_run(lib, pkg, so, xs, smap, S, fz_rel, z_ground, d=None, k=None, mu=0.0):
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, fz_rel, z_ground, d, None if k is None else k[b], mu) for b in range(xs.shape[0])]
    return emu_result(pkg, outs, d is not None or k is not None, mu > 0)


def library_run(pkg, solver, xs, n_steps, S, fz_rel, z_ground, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=(fz_rel, z_ground))


# ---- the cases of tests/test_contact_host.py and tests/test_contact_gpu.py, sized on the CPU with the reference alone.  z_ground = 0 throughout.
# What shaped them: once a foot of this fixture is free, the closed loop is violently unstable.  Without a torque limit the policy answers a free
# foot with forces of 1e4 .. 1e9 N and the sample diverges within ten steps; a 1e-12 change of x0 then grows by 1e6 .. 1e9 x to the end of the
# window.  The largest force of a case sets grf_common.force_bound, and with it the margin every sample needs.  So:
#   - fz_rel = -10 N: sample (2, 2) pulls with 6 N in its first steps without any kick; at fz_rel = 0 it is released at step 0 and lost by step 6;
#   - the kicked cases limit the torque at 8 N m (case D's limit; no noise: still the kernel without the generator), which keeps every force
#     below 120 N and every sample alive;
#   - the kicks come late in the window, so that the events are inside it and it ends before the differences grow (the amplification is measured
#     and bounded by tests/test_contact_host.py).
#   flight      an upward base kick (coordinate 20, rising from 0 to 1.6 m/s over the eight samples) at step 44, a trot stance step; S = 1 and 4.
#               The harder kicked samples release both stance feet, fly and land again; sample 0 of every problem is not kicked.
#   roll        case D's switches (noise, torque limit, fall height), S = 4: a lateral kick (coordinate 19, 0 .. 4 m/s) at step 42 tips the robot
#               over one stance foot: the other one is released alone
#   partial     3 problems x 3 samples, S = 5: the flight kick on a partial wave
#   divergence  2 x 2 samples, S = 4, no limit: sample (1, 1) gets a roll rate of 1e4 rad/s at step 5 and fails the divergence test in substep 1
CASES = [("flight", 1), ("flight", 4), ("roll", 4), ("partial", 5), ("divergence", 4)]
FZ_REL = -10.0


def case_setup(pkg, case, xs):
    """(x0, Disturbance or None, kick or None, fz_rel, z_ground) of a case on the fixture's samples xs [4, 8, 36]."""
    Dist = pkg.sim.Disturbance
    ramp = np.linspace(0.0, 1.0, 8)[None, :]
    if case == "flight":
        k = np.zeros(xs.shape); k[..., 20] = 1.6 * ramp
        return xs, Dist(seed=mc.SEED, u_max=8.0, kick_step=44), k, FZ_REL, 0.0
    if case == "roll":
        D = mc.cases(pkg, xs.shape[:2])["D"][0]
        k = np.zeros(xs.shape); k[..., 19] = 4.0 * ramp
        return xs, Dist(seed=mc.SEED, sigma_u=D.sigma_u, sigma_q=D.sigma_q, sigma_v=D.sigma_v, u_max=D.u_max, fall_height=D.fall_height, kick_step=42), k, FZ_REL, 0.0
    if case == "partial":
        x0 = np.ascontiguousarray(xs[:3, 5:8])
        k = np.zeros(x0.shape); k[..., 20] = 1.6 * ramp[:, 5:8]
        return x0, Dist(seed=mc.SEED, u_max=8.0, kick_step=44), k, FZ_REL, 0.0
    if case == "divergence":
        x0 = np.ascontiguousarray(xs[:2, :2])
        k = np.zeros(x0.shape); k[1, 1, 23] = 1e4
        return x0, Dist(seed=mc.SEED, kick_step=5), k, FZ_REL, 0.0
    raise KeyError(case)


def assert_case_is_not_vacuous(case, ref, contact):
    """What the case is for, asserted on the reference alone."""
    r = ref["rows"]
    flight = (~ref["att"].any(axis=-1) & ref["counted"] & (np.asarray(contact).sum(axis=-1) > 0)[None, None, :, None]).any(axis=(-2, -1))      # every attached foot released
    if case in ("flight", "partial"):
        assert (flight & (r["n_land"] > 0)).any(), "no sample releases every attached foot and lands again"
    if case == "flight":
        assert ((r["n_release"] == 0) & (r["n_land"] == 0) & (r["n_free"] == 0)).any(), "no sample without an event"
    if case == "roll":
        assert ((r["n_release"] == 1) & ~flight & (ref["first_bad"] < 0)).any(), "no sample releases exactly one foot while another stays attached"
    if case == "divergence":
        assert ref["first_bad"][1, 1] == 5 and ref["counted"][1, 1, 5, 1] and not ref["counted"][1, 1, 5, 2:].any() and (ref["first_bad"].ravel()[:3] == -1).all()
