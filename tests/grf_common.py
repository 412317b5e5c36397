"""Shared by tests/test_grf_host.py and tests/test_grf_gpu.py: the reference of the contact-force records (include/hsddp_grf.h) and the comparison
against it.

Reference forces of sample r: on an oracle handle that has solved the problem, set_initial_condition(x0[:, r]) and hybrid_rollout(0.0, MS = 0), then
field(i, "Y") at the window's knots (sim_common.step_map / window) - the route sim_common.oracle_reference takes for X and U.  The reference rows are
sim.grf_rows of those forces.

Tolerances.  Forces: sim_common.RTOL = 1e-8 x max(1, |Y_ref|max), the project's rollout tolerance, which test_per_iterate_parity applies to Y.  That
bound in newtons is the FORCE BOUND; min_fz, min_cone and max_fz are held to it too (they are entries, or differences of entries, of Y).  first_slip
and n_slip are integers of thresholds and are compared EXACTLY, which rests on a precondition the comparison asserts (never skips on): over all stance
(foot, step) pairs of the reference, min |cone| and min |fz - fz_min| are at least 1000 x the force bound, so no pair can change sides within the
bound."""
import numpy as np

import sim_common as sc
import walk_ref as wr
from conftest import pkg

MARGIN_FACTOR = 1000.0


def contact_of(phases, smap):
    """[n, 4]: 1 where foot l is a stance foot of the phase of step s."""
    return np.array([[1 if phases[p]["desc"].contact[l] > 0 else 0 for l in range(4)] for p in smap[0]], dtype=np.int32)


def oracle_forces(so, opt_ss, x0, smap):
    """so: a solved oracle handle of batch B; x0: [B, R, 36].  Returns Y [B, R, n, 12] of the window."""
    nph = len(so.phases)
    B, R = x0.shape[:2]
    Y = np.zeros((B, R, smap.shape[1], 12))
    for r in range(R):
        so.set_initial_condition(np.ascontiguousarray(x0[:, r]))
        so.hybrid_rollout(0.0, opt_ss)
        Y[:, r] = sc.window([so.field(i, "Y") for i in range(nph)], smap, False)
    return Y


def force_bound(Yref):
    return sc.RTOL * max(1.0, float(np.abs(Yref).max()))


def margins(Y, contact, mu, fz_min, first_bad=None):
    """(min |cone|, min |fz - fz_min|) over the stance (foot, step) pairs of Y [..., n, 12] that count (see sim.grf_rows)."""
    n = Y.shape[-2]
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    st = np.broadcast_to(np.asarray(contact).reshape(n, 4) > 0, F.shape[:-1])
    if first_bad is not None:
        fb = np.asarray(first_bad).reshape(Y.shape[:-2] + (1, 1))
        st = st & ((fb < 0) | (np.arange(n).reshape(n, 1) <= fb))
    cone = mu * F[..., 2] - np.maximum(np.abs(F[..., 0]), np.abs(F[..., 1]))
    return float(np.abs(cone[st]).min()), float(np.abs(F[..., 2][st] - fz_min).min())


def assert_swing_is_zero(tag, Y, contact):
    F = Y.reshape(Y.shape[:-1] + (4, 3))
    sw = np.broadcast_to((np.asarray(contact) == 0)[..., None], F.shape)
    assert sw.any(), tag
    assert (F[sw] == 0.0).all(), f"{tag}: a swing leg's force entry is not exactly 0"


def compare_records(tag, pkg, rows, Y, Yref, contact, mu, fz_min):
    """rows (structured, GRF_ROW_DTYPE) and Y (or None) of the backend under test against the reference forces Yref.  Returns the reference rows."""
    bound = force_bound(Yref)
    scale = bound / sc.RTOL
    ref = pkg.sim.grf_rows(Yref, contact, mu, fz_min)
    mc, mf = margins(Yref, contact, mu, fz_min)
    print(f"[grf] {tag}: mu {mu}, force scale {scale:.3e} N, force bound {bound:.3e} N, reference margins min|cone| {mc:.3e} N, min|fz - fz_min| {mf:.3e} N "
          f"(needed {MARGIN_FACTOR * bound:.3e}), slipping samples {int((ref['first_slip'] >= 0).sum())} of {ref.size}, n_slip total {int(ref['n_slip'].sum())}, "
          f"min fz {ref['min_fz'].min():.4f} N")
    assert mc >= MARGIN_FACTOR * bound and mf >= MARGIN_FACTOR * bound, f"{tag}: the reference is within {MARGIN_FACTOR:.0f} x the force bound of a threshold ({mc:.3e}, {mf:.3e})"
    if Y is not None:
        sc.close(tag + " Y", Y, Yref)
        assert_swing_is_zero(tag, Y, contact)
    for f in ("min_fz", "min_cone", "max_fz"):
        sc.close(f"{tag} {f}", rows[f], ref[f], scale=scale)
    assert np.array_equal(rows["first_slip"], ref["first_slip"]), (tag, rows["first_slip"], ref["first_slip"])
    assert np.array_equal(rows["n_slip"], ref["n_slip"]), (tag, rows["n_slip"], ref["n_slip"])
    return ref


def oracle_walk_forces(oracle_lib, phases, policy, smap, x0, psi_dyn=3.1415):
    """The undisturbed window walked knot by knot (walk_ref.reference_walk, one solve per step, no contact rule) with the policy rows given as arrays
    (mc_common.policy_of), keeping the contact forces the probe returns.  x0: [B, R, 36].  Returns Y [B, R, n, 12]."""
    w = wr.reference_walk(pkg, oracle_lib, phases, policy, smap, x0, psi_dyn=psi_dyn)
    assert (w["first_bad"] < 0).all()
    return np.ascontiguousarray(w["Y"][..., 0, :])
