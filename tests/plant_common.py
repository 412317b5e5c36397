"""Shared by tests/test_plant_host.py and tests/test_plant_gpu.py: the references of closed-loop windows with a PER-SAMPLE PLANT (include/hsddp_plant.h),
the host build of the ten programs (tests/_emu/plant_emu.cpp) behind numpy arguments, and the cases.

Reference.  The oracle with link constants that can be varied (tests/_emu/plant_ref.cpp: the whole oracle plus plant_ref_set, built into a temporary
directory with the oracle's own flags - a library of its own, so the oracle the solves run on is never touched), and walk_ref.reference_walk with a plant:
    oracle_walk_sub_plant   sub_common.oracle_walk_sub     the bilateral walks
    oracle_walk_ter_plant   ter_common.oracle_walk_ter     the walks with terrain; with a one-cell flat map and early = 0 the walks with the contact rule alone
                                                            (tests/test_terrain_host.py holds that equality)
with three additions each: the sample's links are set before its walk, every solve is given  gain o u - damping o x[24:36]  of the state it starts from,
and the nominal links are restored at the end.  tests/test_plant_host.py holds both to the walks without a plant bit for bit at a nominal table.

Tolerances: the project's own, unchanged - sim_common.RTOL x scale on trajectories and summaries, grf_common.force_bound on forces, integers exactly, at
most one sample of a case left out for lying within MARGIN_FACTOR x bound of a decision, asserted on the reference alone (uni_common.near_samples,
mc_common.NEAR)."""
import ctypes as C

import numpy as np

import sim_common as sc
import mc_common as mc
import sub_common as sub
import uni_common as un
import ter_common as tc
import walk_ref as wr
from walk_ref import DP, IP, _dp, set_links

W_TD = tc.W_TD


def build_ref(pkg, tmpdir):
    """The oracle with plant_ref_set (tests/_emu/plant_ref.cpp), with the flags of oracle/Makefile."""
    lib = pkg._abi.bind(wr.build_so(tmpdir, "plant_ref.cpp", "liboracle_plant_ref.so", wr.ORACLE_FLAGS))
    lib.plant_ref_set.argtypes = [DP, DP]; lib.plant_ref_set.restype = None
    set_links(lib, np.array(pkg._abi.PLANT_NOMINAL))
    return lib


def oracle_walk_sub_plant(pkg, ref_lib, phases, policy, smap, x0, S, plant, dist=None, kick=None):
    """sub_common.oracle_walk_sub with a plant row per sample.  Returns the same dict."""
    return wr.pick(wr.reference_walk(pkg, ref_lib, phases, policy, smap, x0, S, plant=plant, dist=dist, kick=kick), wr.KEYS_SUB)


def oracle_walk_ter_plant(pkg, ref_lib, phases, policy, smap, x0, S, fz_rel, z_ground, ter, plant, dist=None, kick=None, F0=None, E0=None):
    """ter_common.oracle_walk_ter with a plant row per sample (ter None: the flat one-cell map, early = 0 - the contact rule alone).  Returns the same dict."""
    w = wr.reference_walk(pkg, ref_lib, phases, policy, smap, x0, S, contact=(fz_rel, z_ground), ter=ter, plant=plant, dist=dist, kick=kick, F0=F0, E0=E0)
    return wr.pick(w, wr.KEYS_TER)


def impact_ref(pkg, ref_lib, desc, x, row):
    """The reset map of the phase `desc` on the state x [36] with the links of `row`."""
    ct = np.array([desc.contact[l] for l in range(4)], dtype=np.int32); nx = np.array([desc.next_contact[l] for l in range(4)], dtype=np.int32)
    xi = np.zeros(36)
    try:
        set_links(ref_lib, row)
        ref_lib.oracle_wb_impact(_dp(np.ascontiguousarray(x, dtype=np.float64)), ct.ctypes.data_as(IP), nx.ctypes.data_as(IP), C.c_double(mc.PSI_DYN), C.c_double(np.pi), 1, _dp(xi), None)
    finally:
        set_links(ref_lib, np.array(pkg._abi.PLANT_NOMINAL))
    return xi


# ---- the host build of the ten programs

def build_emu(tmpdir):
    lib = wr.build_so(tmpdir, "plant_emu.cpp", "libhsddp_plant_emu.so")
    # the parked column is that of the twin with records and sub-step loop: nothing of the row is parked
    assert [lib.plant_emu_park_doubles(m, f) for f in (0, 1, 2) for m in (0, 1)] == [32, 34, 39, 41, 45, 47] and lib.plant_emu_row_doubles() == 46
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, plant_rows, plant_of=None, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, map_of=None, dist=None, kick=None, mu=0.0, fz_min=0.0,
            F=None, E=None, hold=None, expect=0):
    """The host build on problem b of a solved handle; x0, kick: [R, 36]; plant_rows [n_plants, 46], plant_of None or int [R]; family "bi", "uni" or
    "ter".  Returns raw arrays (expect != 0: the return code the call must give, and None)."""
    R = x0.shape[0]
    args, out, keep = wr.emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min)
    ctail, out["c"] = wr.emu_contact_args(R, fz_rel, z_ground, F, hold, E)
    ttail, out["t"] = wr.emu_terrain_args(R, ter, map_of, E)
    if family != "ter":      # (only the terrain family is given the terrain's parameters)
        ttail[0] = None
    P = None if plant_rows is None else np.ascontiguousarray(plant_rows, dtype=np.float64)
    po = None if plant_of is None else np.ascontiguousarray(plant_of, dtype=np.int32)
    rc = lib.plant_emu_run(*args, 0 if family == "bi" else 1, *ctail, *ttail, 0 if P is None else (P.shape[0] if P.ndim == 2 else 1), wr.vp(P), wr.vp(po))
    assert rc == expect, (rc, expect)
    return None if expect else out


def host_run(lib, pkg, so, xs, smap, S, plant, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, d=None, k=None, mu=0.0):
    P = plant.table()
    po = None if plant.plant_of is None else np.asarray(plant.plant_of)
    mo = None if ter is None or ter.map_of is None else np.asarray(ter.map_of)
    outs = [emu_run(lib, pkg, so, b, xs[b], smap, S, P, None if po is None else po[b], family, fz_rel, z_ground, ter, None if mo is None else mo[b], d, None if k is None else k[b], mu)
            for b in range(xs.shape[0])]
    dis = d is not None or k is not None
    if family == "bi":
        return sub.emu_result(pkg, outs, dis, mu > 0)
    res = un.emu_result(pkg, outs, dis, mu > 0)
    if family == "ter":
        res["terrain"] = tc.terrain_rows_of(pkg, np.stack([o["t"] for o in outs]))
    return res


def library_run(pkg, solver, xs, n_steps, S, plant, family="bi", fz_rel=0.0, z_ground=0.0, ter=None, d=None, k=None, mu=0.0):
    """The same run through the library's Python layer (plant None: the plant off)."""
    return solver.simulate(xs, n_steps, keep_traj=True, dist=d, kick=k, grf=(mu, 0.0) if mu > 0 else None, substeps=S, contact=None if family == "bi" else (fz_rel, z_ground),
                           terrain=ter if family == "ter" else None, plant=plant)


def compare_bilateral(tag, pkg, res, ref, xbar, contact, mu, fz_min=0.0):
    """One bilateral run with the plant on against oracle_walk_sub_plant.  The window, the forces and the three float records of EVERY sample (no decision
    feeds back into a bilateral walk); first_slip, n_slip, first_fall and n_sat exactly, but for the samples whose REFERENCE passes within
    MARGIN_FACTOR x the force bound of a record threshold or within mc_common.NEAR of a torque or height threshold: at most ONE per case, asserted on the
    reference before anything is compared.  (sub_common.compare_records_sub asks for that margin of every sample: the payload rows put one (foot,
    substep) pair of the plain cases at 0.8 / 0.95 of it, so the cap of one that the walks with decisions use is applied here too.)  Returns the mask."""
    import grf_common as gc
    Yref = ref["Y"]
    n, S = Yref.shape[-3], Yref.shape[-2]
    bound = gc.force_bound(Yref); scale = bound / sc.RTOL
    F = Yref.reshape(Yref.shape[:-1] + (4, 3))
    st = np.broadcast_to((np.asarray(contact).reshape(n, 1, 4) > 0), F.shape[:-1]) & np.asarray(ref["counted"])[..., None]
    cone = mu * F[..., 2] - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    margin = np.minimum(np.where(st, np.abs(cone), np.inf), np.where(st, np.abs(F[..., 2] - fz_min), np.inf)).min(axis=(-3, -2, -1))
    near = margin < gc.MARGIN_FACTOR * bound
    if "extra" in res:
        near = near | (ref["sat_margin"] < mc.NEAR) | (ref["fall_margin"] < mc.NEAR)
    print(f"[plant] {tag}: force bound {bound:.3e} N (needed margin {gc.MARGIN_FACTOR * bound:.3e}), smallest record margin {margin.min():.3e} N, two smallest per sample "
          f"{np.sort(margin.ravel())[:2]}, left out {int(near.sum())} of {near.size}")
    assert near.sum() <= 1, f"{tag}: {int(near.sum())} samples of the reference lie within the margin of a decision"
    keep = ~near
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    if "extra" in res:
        assert np.array_equal(res["extra"]["n_sat"][keep], ref["n_sat"][keep]) and np.array_equal(res["extra"]["first_fall"][keep], ref["first_fall"][keep]), tag
    want = pkg.sim.grf_rows_sub(Yref, contact, mu, fz_min, counted=ref["counted"])
    if res.get("Y") is not None:
        sc.close(tag + " Y", res["Y"], Yref[..., 0, :])
        gc.assert_swing_is_zero(tag, res["Y"], contact)
    for f in ("min_fz", "min_cone", "max_fz"):
        sc.close(f"{tag} {f}", res["grf"][f], want[f], scale=scale)
    assert np.array_equal(res["grf"]["first_slip"][keep], want["first_slip"][keep]), (tag, res["grf"]["first_slip"], want["first_slip"])
    assert np.array_equal(res["grf"]["n_slip"][keep], want["n_slip"][keep]), (tag, res["grf"]["n_slip"], want["n_slip"])
    return near


# ---- the tables and the cases, on the fixture of the contact and terrain tests (trot 4 x 12, B = 4, R = 8 around Xbar[0], 48 steps), sized on the CPU
# with the reference alone (the margins are in the docstrings of the tests that use them)

def three_rows(pkg):
    """Nominal; a 1 kg payload at (0.05, 0, 0.04); a 2 kg payload at (0.08, 0.03, 0.05) with link_scale (0.8, 1.2, 1.1) on every leg."""
    s = pkg.sim
    nom = s.Plant.nominal().rows[0]
    return np.stack([nom, s.with_trunk(nom, *s.payload_trunk(1.0, (0.05, 0.0, 0.04))), s.with_link_scale(s.with_trunk(nom, *s.payload_trunk(2.0, (0.08, 0.03, 0.05))), (0.8, 1.2, 1.1))])


def mixed_table(pkg, shape, rows=None, index=lambda b, r: b + r):
    """The three rows with plant_of[b, r] = index(b, r) mod 3, (b + r) mod 3 unless a case says otherwise."""
    po = index(np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]) % 3
    return pkg.sim.Plant(three_rows(pkg) if rows is None else rows, plant_of=po.astype(np.int32))


def gain_damping_rows(pkg, rows):
    """`rows` with the gains linspace(0.8, 1.1, 12) and b = 0.01 on the non-nominal ones."""
    out = np.array(rows, dtype=np.float64)
    for i in range(1, out.shape[0]):
        out[i] = pkg.sim.with_damping(pkg.sim.with_gain(out[i], np.linspace(0.8, 1.1, 12)), 0.01)
    return out


def assert_table_moves_the_reference(tag, ref, ref_nominal, plant):
    """Non-vacuity, on the references alone: every sample of a non-nominal row moves by more than 1e-3 in X."""
    po = np.asarray(plant.plant_of)
    nominal_row = np.array([np.array_equal(r, plant.table()[0]) for r in plant.table()])
    moved = np.abs(ref["X"] - ref_nominal["X"]).max(axis=(-2, -1))
    off = ~nominal_row[po]
    print(f"[plant] {tag}: |X - X_nominal| of the samples of a non-nominal row {moved[off].min():.3e} .. {moved[off].max():.3e}, of a nominal row {moved[~off].max() if (~off).any() else 0.0:.3e}")
    assert off.any() and (moved[off] > 1e-3).all(), (tag, moved)
    assert not moved[~off].any()


# (family, case, S, table): the bilateral walks plain (k_sim_quad_plant) and under case D's switches with gains and friction (k_sim_quad_mc_plant); the
# contact rule on the flight kick (k_sim_quad_mc0_uni_plant), under case D's noise with the roll kick (k_sim_quad_mc_uni_plant), on a partial wave and with
# the contained divergence; the block and a map per sample under noise (k_sim_quad_mc0_ter_plant, k_sim_quad_mc_ter_plant).  "mixed": plant_common.mixed_table; "mixed2": the same rows with plant_of = (2 b + r + 2) mod 3 -
# the block's early touchdowns are many close decisions: "mixed" puts TWO samples of the reference within the margin of a landing test (2.4e-7 and 3.2e-6
# against 1e-5), and so do six other index maps tried on the CPU ((b + r + 1), (b + r + 2) with the records, (b + 2 r + 0 .. 2), (2 b + r), (2 b + r + 1):
# two or three); this one leaves out one sample, for a record threshold.
CASES = [("bi", "plain", 1, "mixed"), ("bi", "plain", 3, "mixed"), ("bi", "D", 4, "gains"), ("uni", "flight", 4, "mixed"), ("uni", "roll", 4, "mixed"), ("uni", "partial", 5, "mixed"),
         ("uni", "divergence", 4, "mixed"), ("ter", "block", 4, "mixed2"), ("ter", "maps", 4, "mixed")]


def case_of(pkg, family, case, S, table, xs):
    """(x0, dist, kick, fz_rel, z_ground, terrain, Plant) of a case on the fixture's samples."""
    if family == "bi":
        d, k = (None, None) if case == "plain" else mc.cases(pkg, xs.shape[:2])["D"][:2]
        x0, fz_rel, zg, ter = xs, 0.0, 0.0, None
    elif family == "uni":
        x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs); ter = None
    else:
        x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
    pl = mixed_table(pkg, x0.shape[:2])
    if table == "mixed2":
        pl = mixed_table(pkg, x0.shape[:2], index=lambda b, r: 2 * b + r + 2)
    if table == "gains":
        pl = pkg.sim.Plant(gain_damping_rows(pkg, pl.rows), plant_of=pl.plant_of)
    return x0, d, k, fz_rel, zg, ter, pl


def reference_of(pkg, ref_lib, phases, pol, smap, family, x0, S, fz_rel, zg, ter, pl, d, k):
    if family == "bi":
        return oracle_walk_sub_plant(pkg, ref_lib, phases, pol, smap, x0, S, pl, d, k)
    return oracle_walk_ter_plant(pkg, ref_lib, phases, pol, smap, x0, S, fz_rel, zg, ter, pl, d, k)


def compare(pkg, tag, family, res, ref, xbar, contact, mu, fz_rel):
    if family == "bi":
        return compare_bilateral(tag, pkg, res, ref, xbar, contact, mu)
    if family == "uni":
        return un.compare_case(tag, pkg, res, ref, xbar, mu, 0.0, fz_rel)
    return tc.compare_case(tag, pkg, res, ref, xbar, mu, 0.0, fz_rel)


def bad_tables(pkg):
    """(rows, plant_of) pairs hsddp_plant_set refuses, for a batch of 4 x 2 samples; the first entry of each pair may be None."""
    nom = np.array(pkg._abi.PLANT_NOMINAL)
    P = np.stack([nom, nom, nom])
    po = (np.arange(8) % 3).astype(np.int32)

    def put(i, j, v):
        Q = P.copy(); Q[i, j] = v
        return Q
    bad = [(None, po), (put(0, 0, 0.0), po), (put(1, 0, -2.0), po), (put(2, 3, np.nan), po), (put(0, 45, np.inf), po), (put(1, 22, -np.inf), po), (put(0, 4, 0.0), po),
           (put(1, 5, 0.03), po), (put(2, 9, -0.01), po), (put(0, 8, 0.05), po), (put(1, 13, 0.0), po), (put(2, 21, -0.5), po), (put(0, 34, -1e-9), po)]
    for v in (-1, 3):
        q = po.copy(); q[7] = v
        bad.append((P, q))
    return P, po, bad
