"""Shared by tests/test_substep_host.py and tests/test_substep_gpu.py: the reference of a SUB-STEPPED closed-loop window (include/hsddp_substep.h),
the host build of the sub-stepped program (tests/_emu/sub_emu.cpp) behind numpy arguments, and the comparison against the reference.

Reference: walk_ref.reference_walk with S substeps and no contact rule; it keeps the force of every substep, Y [B, R, n, S, 12], and the mask
`counted` [B, R, n, S] (the sample was alive when the substep began).  Policy rows come from the handle under test (mc_common.policy_of).

Tolerances.  X, U, x_final and the summaries: sim_common.compare_window, RTOL = 1e-8 x scale (a 1e-12 change of x0 grows by 66 x in X and 390 x in Y
through the 48-step window at S = 2, 3 and 4 alike, measured on the CPU).  Forces and the three float records: grf_common.force_bound.  first_slip
and n_slip EXACTLY, under grf_common's precondition, asserted: every counted stance (foot, substep) pair of the reference lies >= 1000 x the force
bound from both thresholds.  first_fall and n_sat: mc_common.compare_extra (exactly, at most one sample per case within NEAR of a threshold left out)."""
import numpy as np

import sim_common as sc
import mc_common as mc
import grf_common as gc
import walk_ref as wr


def oracle_walk_sub(pkg, oracle_lib, phases, policy, smap, x0, S, dist=None, kick=None):
    """x0: [B, R, 36]; S: substeps per control step.  Returns what mc_common.oracle_walk returns - X [B, R, n + 1, 36], U [B, R, n, 12], first_bad,
    first_fall, n_sat, sat_margin, fall_margin [B, R] - and Y [B, R, n, S, 12], counted [B, R, n, S]."""
    return wr.pick(wr.reference_walk(pkg, oracle_lib, phases, policy, smap, x0, S, dist=dist, kick=kick), wr.KEYS_SUB)


def sub_margins(Y, contact, mu, fz_min, counted):
    """(min |cone|, min |fz - fz_min|) over the counted stance (foot, substep) pairs of Y [..., n, S, 12]."""
    n, S = Y.shape[-3], Y.shape[-2]
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    st = np.broadcast_to((np.asarray(contact).reshape(n, 1, 4) > 0), F.shape[:-1]) & np.asarray(counted)[..., None]
    cone = mu * F[..., 2] - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    return float(np.abs(cone[st]).min()), float(np.abs(F[..., 2][st] - fz_min).min())


def compare_records_sub(tag, pkg, rows, Y, ref, contact, mu, fz_min):
    """rows (GRF_ROW_DTYPE) and Y [B, R, n, 12] (or None) of the backend under test against the reference walk `ref` (oracle_walk_sub): forces of
    substep 0 and the three floats within the force bound, first_slip and n_slip EQUAL under the asserted margin precondition.  Returns the
    reference rows."""
    Yref = ref["Y"]
    bound = gc.force_bound(Yref)
    scale = bound / sc.RTOL
    want = pkg.sim.grf_rows_sub(Yref, contact, mu, fz_min, counted=ref["counted"])
    mcone, mfz = sub_margins(Yref, contact, mu, fz_min, ref["counted"])
    print(f"[sub] {tag}: S {Yref.shape[-2]}, mu {mu}, force scale {scale:.3e} N, force bound {bound:.3e} N, reference margins min|cone| {mcone:.3e} N, "
          f"min|fz - fz_min| {mfz:.3e} N (needed {gc.MARGIN_FACTOR * bound:.3e}), slipping samples {int((want['first_slip'] >= 0).sum())} of {want.size}, "
          f"n_slip total {int(want['n_slip'].sum())}, min fz {want['min_fz'].min():.4f} N")
    assert mcone >= gc.MARGIN_FACTOR * bound and mfz >= gc.MARGIN_FACTOR * bound, \
        f"{tag}: the reference is within {gc.MARGIN_FACTOR:.0f} x the force bound of a threshold ({mcone:.3e}, {mfz:.3e})"
    if Y is not None:
        sc.close(tag + " Y", Y, Yref[..., 0, :])
        gc.assert_swing_is_zero(tag, Y, contact)
    for f in ("min_fz", "min_cone", "max_fz"):
        sc.close(f"{tag} {f}", rows[f], want[f], scale=scale)
    assert np.array_equal(rows["first_slip"], want["first_slip"]), (tag, rows["first_slip"], want["first_slip"])
    assert np.array_equal(rows["n_slip"], want["n_slip"]), (tag, rows["n_slip"], want["n_slip"])
    return want


# ---- the host build of the sub-stepped program

def build_emu(tmpdir):
    lib = wr.build_so(tmpdir, "sub_emu.cpp", "libhsddp_sub_emu.so")
    # the parked column of the six sub-stepped kernels: 27 / 29 doubles per lane without records, 32 / 34 with them
    assert [lib.sub_emu_park_doubles(m, g) for m, g in ((0, 0), (1, 0), (0, 1), (1, 1))] == [27, 29, 32, 34]
    return lib


def emu_run(lib, pkg, so, b, x0, smap, S, dist=None, kick=None, mu=0.0, fz_min=0.0, keep_traj=True):
    """The host build on problem b of a solved handle; x0, kick: [R, 36].  S >= 1: the SUB walk; S == 0: the walk without the switch.  dist / kick
    None: the plain walk, else the disturbed one.  mu > 0: with records.  Returns a dict of raw arrays: xf, rows, X, U, extra, g, Y."""
    args, out, keep = wr.emu_prefix(pkg, so, b, x0, smap, S, dist, kick, mu, fz_min, keep_traj)
    assert lib.sub_emu_run(*args) == 0
    return out


def emu_result(pkg, outs, disturbed, records):
    """The per-problem raw outputs of emu_run stacked into the dict the library's Python layer returns (rows, x_final, X, U, extra, grf, Y)."""
    st = lambda k: np.stack([o[k] for o in outs])
    raw = st("rows")
    r = np.zeros(raw.shape[:-1], dtype=pkg._abi.SIM_ROW_DTYPE)
    for i, f in enumerate(("dev_q", "dev_v", "min_height", "max_torque", "first_bad")):
        r[f] = raw[..., i]
    res = dict(rows=r, x_final=st("xf"), X=st("X"), U=st("U"))
    if disturbed:
        ex = st("extra")
        e = np.zeros(ex.shape[:-1], dtype=pkg._abi.MC_EXTRA_DTYPE)
        e["first_fall"] = ex[..., 0]; e["n_sat"] = ex[..., 1]
        res["extra"] = e
    if records:
        res["grf"] = wr.struct_rows(st("g"), pkg._abi.GRF_ROW_DTYPE); res["Y"] = st("Y")
    return res


def compare_case(tag, pkg, res, ref, xbar, contact=None, mu=0.0, fz_min=0.0):
    """One run against its reference walk: the window, the extras of a disturbed run, the records of a run with them."""
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    if "extra" in res:
        mc.compare_extra(tag, res["extra"], ref)
    if "grf" in res:
        compare_records_sub(tag, pkg, res["grf"], res.get("Y"), ref, contact, mu, fz_min)
