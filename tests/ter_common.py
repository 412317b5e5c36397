"""Shared by tests/test_terrain_host.py and tests/test_terrain_gpu.py: the reference of a closed-loop window with TERRAIN HEIGHT MAPS AND EARLY SWING-FOOT
TOUCHDOWN (include/hsddp_terrain.h), the host build of the program (tests/_emu/ter_emu.cpp) behind numpy arguments, and the comparison.

Reference: walk_ref.reference_walk with the contact rule and a terrain, in numpy on the oracle's existing probes only; sim.terrain_height is the
lookup.  The walk is started from given (F, E) and returns, beside what oracle_walk_uni returns, the terrain rows, E at the end, and what the cases
assert their non-vacuity on (the raw cell indices and the cells of the tested feet).

Tolerances: the project's own, uni_common's.  Floats 1e-8 x scale (sim_common / grf_common), the integers, free_final and early_final EXACTLY, but
for a sample whose REFERENCE comes within grf_common.MARGIN_FACTOR x the bound of a decision; at most ONE such sample per case (uni_common.near_samples
asserts it on the reference).  The decisions and their margins: the two kinds of uni_common (force_margin, kin_margin), and folded into kin_margin
(all are metres or metres per second against the trajectory bound 1e-8):
  - a swing foot's landing test (p_z <= z_g and w_z < -w_td): true - the smaller of |p_z - z_g| and |w_z + w_td|; false - the larger over the
    conditions that fail;
  - for a tested foot whose neighbouring cell holds a different height: the distance of p_x / p_y to that cell edge."""
import numpy as np

import sim_common as sc
import uni_common as un
import walk_ref as wr

INTS_T = ("first_early", "n_early", "n_early_release", "n_held", "early_final")


def oracle_walk_ter(pkg, oracle_lib, phases, policy, smap, x0, S, fz_rel, z_ground, ter, dist=None, kick=None, F0=None, E0=None):
    """x0: [B, R, 36]; ter: sim.Terrain (map_of None or [B, R]); F0, E0: None or bool [B, R, 4].  Returns the dict of uni_common.oracle_walk_uni (att
    holds the feet of E too) plus trows (TERRAIN_ROW_DTYPE [B, R]), E [B, R, 4] at the end, raw_ix / raw_iy (smallest and largest raw cell index of a
    tested foot), cells (the set of (m, iy, ix) a tested foot read), pz_final [B, R, 4] (foot heights of the final state), land_z [B, R, 2] (lowest and highest p_z of a foot of a landing set T; NaN: none)."""
    w = wr.reference_walk(pkg, oracle_lib, phases, policy, smap, x0, S, contact=(fz_rel, z_ground), ter=ter, dist=dist, kick=kick, F0=F0, E0=E0)
    return wr.pick(w, wr.KEYS_TER)


def report(tag, ref):
    t, r = ref["trows"], ref["rows"]
    print(f"[ter] {tag}: early touchdowns {int(t['n_early'].sum())} on {int((t['n_early'] > 0).sum())} of {t.size} samples, early releases {int(t['n_early_release'].sum())}, held pairs "
          f"{int(t['n_held'].sum())}, stance releases {int(r['n_release'].sum())}, stance landings {int(r['n_land'].sum())}, max_pen {t['max_pen'].max():.3e}, max_lift {r['max_lift'].max():.3e}, "
          f"raw ix {ref['raw_ix']}, raw iy {ref['raw_iy']}, cells {sorted(ref['cells'])[:8]}, diverged {int((ref['first_bad'] >= 0).sum())}")


def compare_case(tag, pkg, res, ref, xbar, mu=0.0, fz_min=0.0, fz_rel=None):
    """One run with the contact rule and the terrain on against its reference walk: everything uni_common.compare_case holds (the cap of one left-out
    sample is asserted there, on the reference, before anything is compared), then the terrain rows."""
    report(tag, ref)
    near = un.compare_case(tag, pkg, {k: v for k, v in res.items() if k != "terrain"}, ref, xbar, mu, fz_min, fz_rel)
    keep = ~near
    got, want = res["terrain"], ref["trows"]
    for f in INTS_T:
        assert np.array_equal(got[f][keep], want[f][keep]), (tag, f, got[f], want[f])
    sc.close(f"{tag} max_pen", got["max_pen"][keep], want["max_pen"][keep], scale=1.0)
    return near


# ---- the host build of the program

def build_emu(tmpdir):
    lib = wr.build_so(tmpdir, "ter_emu.cpp", "libhsddp_ter_emu.so")
    assert [lib.ter_emu_park_doubles(m) for m in (0, 1)] == [45, 47]      # the parked column of the three kernels, doubles per lane: 24 064 B at most
    return lib


def emu_args(pkg, so, b, x0, smap):
    """The policy arguments of the host builds for problem b of a solved handle: walk_ref.policy_arrays."""
    return wr.policy_arrays(so, b)


def emu_run(lib, pkg, so, b, x0, smap, S, fz_rel, z_ground, ter, map_of=None, dist=None, kick=None, mu=0.0, fz_min=0.0, F=None, E=None, hold=None, expect=0):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; map_of: None or int [R]; F, E: None or float [R, 4], updated in place.
    Returns raw arrays (expect != 0: the return code the call must give, and None)."""
    R = x0.shape[0]
    args, out, keep = wr.emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min)
    ctail, out["c"] = wr.emu_contact_args(R, fz_rel, z_ground, F, hold, E)
    ttail, out["t"] = wr.emu_terrain_args(R, ter, map_of, E)
    rc = lib.ter_emu_run(*args, *ctail, *ttail)
    assert rc == expect, (rc, expect)
    return None if expect else out


def terrain_rows_of(pkg, raw):
    return wr.struct_rows(raw, pkg._abi.TERRAIN_ROW_DTYPE)


def host_run(lib, pkg, so, xs, smap, S, fz_rel, z_ground, ter, d=None, k=None, mu=0.0):
    mo = None if ter.map_of is None else np.asarray(ter.map_of)
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, fz_rel, z_ground, ter, None if mo is None else mo[b], d, None if k is None else k[b], mu) for b in range(xs.shape[0])]
    res = un.emu_result(pkg, outs, d is not None or k is not None, mu > 0)
    res["terrain"] = terrain_rows_of(pkg, np.stack([o["t"] for o in outs]))
    return res


def library_run(pkg, solver, xs, n_steps, S, fz_rel, z_ground, ter, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=(fz_rel, z_ground), terrain=ter)


# ---- the cases of tests/test_terrain_host.py and tests/test_terrain_gpu.py, on the contact tests' fixture (uni_common: trot 4 x 12, B = 4, R = 8 around
# Xbar[0], 48 steps, fz_rel = -10 N, u_max = 8 N m, the "flight" kick at step 44; z_ground = 0), sized on the CPU with the reference alone.  The planned
# stance feet of the fixture stand at z = 0; its swing feet clear the ground by a few centimetres, so a step of +3 cm is met by most of them.
#   flat        H = 0, early = 0, S = 3: the walk of uni_common's flight case, to be compared with the run without the terrain
#   block       one map of two cells of 10 m, the second from x = 0.15 m on 3 cm higher: the front feet (x = +0.19 +- the stride) cross the riser, the
#               hind feet stay on the low cell; early = 1, w_td = 0.05 m/s; S = 1 and 4
#   maps        three one-cell maps - flat, +3 cm, -2 cm - with map_of[b, r] = (b + r) mod 3, under case D's noise switches (k_sim_quad_mc_ter), S = 4
#   edge        3 problems x 3 samples (a partial wave), S = 5, a 4 x 4 grid of 5 cm cells around the origin with a chequered +-5 mm: every foot is
#               outside the grid, on every side, and reads an edge cell
#   divergence  uni_common's contained divergence on the block terrain
#   episode     (tests/test_terrain_gpu.py) the window of episode_phases: the trot without its leading stance phase, so that every tick of 11 steps
#               starts in a swing phase and ends one knot before its touchdown, where the swing feet that met the block are held: with the same policy
#               the reference ends tick 0 with E = {0} or {0, 3} on all four robots and counts 87 .. 88 held pairs in tick 1.  The block is 2.5 cm
#               here: at 3 cm two of the four robots come within 5.4e-6 and 5.7e-6 of a landing test in tick 0 (the cap is one); at 2.5 cm the
#               smallest landing margin of the three ticks is 1.8e-4, the smallest force margin 1.9 N
W_TD = 0.05
CASES = [("block", 1), ("block", 4), ("maps", 4), ("edge", 5), ("divergence", 4)]


def terrain_of(pkg, case, shape):
    T = pkg.sim.Terrain
    if case == "flat":
        return T(H=np.zeros((1, 1, 1)), early=False)
    if case in ("block", "divergence", "episode"):
        return T(H=np.array([[[0.0, 0.025 if case == "episode" else 0.03]]]), x0=-9.85, y0=-5.0, cx=10.0, cy=10.0, early=True, w_td=W_TD)
    if case == "maps":
        mo = (np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 3
        return T(H=np.array([0.0, 0.03, -0.02]).reshape(3, 1, 1), early=True, w_td=W_TD, map_of=mo.astype(np.int32))
    if case == "edge":
        i = np.arange(4)
        return T(H=0.005 * np.where((i[:, None] + i[None, :]) % 2 == 0, 1.0, -1.0)[None], x0=-0.1, y0=-0.1, cx=0.05, cy=0.05, early=True, w_td=W_TD)
    raise KeyError(case)


def episode_phases(pkg):
    return pkg.problems.wb_trot_problem(schedule=((0, 1, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 0, 0, 1)), horizons=(12, 12, 12, 12), last_next=(0, 1, 1, 0))


def case_setup(pkg, case, xs):
    """(x0, Disturbance, kick, fz_rel, z_ground, Terrain) of a case on the fixture's samples xs [4, 8, 36]."""
    if case == "maps":      # case D's switches with the flight kick
        x0, d, k, fz_rel, zg = un.case_setup(pkg, "roll", xs)
        _, df, k, _, _ = un.case_setup(pkg, "flight", xs)
        d = pkg.sim.Disturbance(seed=d.seed, sigma_u=d.sigma_u, sigma_q=d.sigma_q, sigma_v=d.sigma_v, u_max=df.u_max, fall_height=d.fall_height, kick_step=df.kick_step)
    else:
        x0, d, k, fz_rel, zg = un.case_setup(pkg, {"flat": "flight", "block": "flight", "edge": "partial", "divergence": "divergence"}[case], xs)
    return x0, d, k, fz_rel, zg, terrain_of(pkg, case, x0.shape[:2])


def assert_case_is_not_vacuous(case, ref, ter):
    """What the case is for, asserted on the reference alone."""
    t, r = ref["trows"], ref["rows"]
    if case == "block":
        assert (t["n_early"] > 0).sum() > t.size // 2, "early touchdowns on fewer than half of the samples"
        assert (t["n_early_release"] > 0).any() and (r["n_release"] > 0).any() and (r["n_land"] > 0).any()
        assert {(0, 0, 0), (0, 0, 1)} <= ref["cells"], "no tested foot in one of the two cells"
    if case == "maps":
        mo = np.asarray(ter.map_of)
        assert all((mo == m).any() for m in range(3)) and (t["n_early"] > 0).any()
    if case == "edge":
        H = ter.grid()
        assert ref["raw_ix"][0] < 0 and ref["raw_ix"][1] > H.shape[2] - 1 and ref["raw_iy"][0] < 0 and ref["raw_iy"][1] > H.shape[1] - 1
        assert (t["n_early"] > 0).any()
    if case == "divergence":
        assert ref["first_bad"][1, 1] == 5 and (ref["first_bad"].ravel()[:3] == -1).all()


def assert_pit_samples_land_lower(ref, ter):
    """Case 3 on the reference: every landing of a sample of the pit map (-2 cm) happens at or below -2 cm, every sample of the flat map has a landing
    above that, and a pit sample that released a stance foot saw it at least 2 cm above its ground (the planned ground is the plane z = 0).  The lowest
    final foot heights are printed: a sample of the pit that never lands keeps walking on the planned plane, held by its scheduled constraints, so
    they do not separate the maps."""
    mo = np.asarray(ter.map_of)
    live = ref["first_bad"] < 0
    pit, flat = (mo == 2) & live, (mo == 0) & live
    top = ref["land_z"][..., 1]
    landed = np.isfinite(top)
    low = np.nanmin(ref["pz_final"], axis=-1)
    print(f"[ter] maps: highest landing, pit samples {top[pit & landed]}, flat samples {top[flat & landed]}; lowest final foot, pit {low[pit].min():.4f} .. {low[pit].max():.4f}, "
          f"flat {low[flat].min():.4f} .. {low[flat].max():.4f}; max_lift of the pit samples with a release {ref['rows']['max_lift'][pit & (ref['rows']['n_release'] > 0)]}")
    assert (pit & landed).sum() >= 2 and (flat & landed).sum() >= 2
    assert top[pit & landed].max() <= -0.02 < top[flat & landed].min()
    rel = pit & (ref["rows"]["n_release"] > 0)
    assert rel.any() and (ref["rows"]["max_lift"][rel] >= 0.02 - 1e-3).all()
