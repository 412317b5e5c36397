"""Shared by tests/test_mc_host.py and tests/test_mc_gpu.py: the reference of a DISTURBED closed-loop window (include/hsddp_mc.h) and the
comparison against it.

Reference: walk_ref.reference_walk with one solve per control step and no contact rule - the window walked knot by knot in numpy, per sample, on the
oracle's model probes.  With every switch off the walk agrees with sim_common.oracle_reference (hybrid_rollout(0, MS = 0)) to 1.5e-13:
test_mc_host.py::test_undisturbed_walk_is_the_oracle_rollout.

Tolerances.  X, U, x_final and the four summaries: sim_common.compare_window, RTOL = 1e-8 x scale, the project's rollout tolerance (a 1e-12 change
of x0 grows by at most 60 x through the disturbed windows used here, so round-off-level differences stay four orders below it).  first_fall and
n_sat are integers of thresholds and are compared EXACTLY, except for a sample whose REFERENCE walk comes within NEAR = 1e-6 (100 x the
trajectory bound) of a threshold - ||u_raw| - u_max| over all joints and steps, |x[2] - fall_height| over all recorded states; at most one
sample of a case may be left out that way."""
import numpy as np

import sim_common as sc
import walk_ref as wr

NEAR = 1e-6
SEED = 20241222
PSI_DYN = wr.PSI_DYN


def policy_of(handle):
    """The policy rows of a solved handle, per phase: XBAR [B, h + 1, 36], UBAR [B, h, 12], K [B, h, 12, 36]."""
    n = len(handle.phases)
    return {f: [handle.field(i, f) for i in range(n)] for f in ("XBAR", "UBAR", "K")}


def xbar_window(policy, smap):
    return sc.window(policy["XBAR"], smap, True)


def oracle_walk(pkg, oracle_lib, phases, policy, smap, x0, dist=None, kick=None):
    """x0: [B, R, 36]; dist: sim.Disturbance or None; kick: [B, R, 36] or None.  Returns dict X [B, R, n + 1, 36], U [B, R, n, 12], first_bad,
    first_fall, n_sat [B, R] and the margins sat_margin, fall_margin [B, R] (inf where the switch is off)."""
    return wr.pick(wr.reference_walk(pkg, oracle_lib, phases, policy, smap, x0, dist=dist, kick=kick), wr.KEYS_MC, read_only=())


def compare_extra(tag, extra, ref):
    """first_fall and n_sat exactly, but for the samples whose reference walk passes within NEAR of a threshold (at most one per case)."""
    near = (ref["sat_margin"] < NEAR) | (ref["fall_margin"] < NEAR)
    print(f"[mc] {tag}: n_sat total {int(ref['n_sat'].sum())} on {int((ref['n_sat'] > 0).sum())} samples, falls {int((ref['first_fall'] >= 0).sum())}, "
          f"nearest torque margin {ref['sat_margin'].min():.3e}, nearest height margin {ref['fall_margin'].min():.3e}, left out {int(near.sum())}")
    assert near.sum() <= 1, tag
    assert np.array_equal(extra["n_sat"][~near], ref["n_sat"][~near]), (tag, extra["n_sat"], ref["n_sat"])
    assert np.array_equal(extra["first_fall"][~near], ref["first_fall"][~near]), (tag, extra["first_fall"], ref["first_fall"])


def compare_disturbed(tag, res, ref, xbar):
    """res: rows, x_final, extra and optionally X, U of the backend under test against the oracle walk `ref`."""
    sc.compare_window(tag, res, ref["X"], ref["U"], xbar)
    compare_extra(tag, res["extra"], ref)


def kick_y(shape, v):
    """The push of the cases below: + v on coordinate 19 (base velocity y) of every sample."""
    k = np.zeros(tuple(shape) + (36,)); k[..., 19] = v
    return k


def cases(pkg, shape):
    """Cases A - D of the 48-step trot window: name -> (Disturbance, kick or None)."""
    Dist = pkg.sim.Disturbance
    return {
        "A": (Dist(seed=SEED, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01), None),
        "B": (Dist(seed=SEED, u_max=8.0), None),
        "C": (Dist(seed=SEED, u_max=6.0, fall_height=0.16, kick_step=10), kick_y(shape, 0.5)),
        "D": (Dist(seed=SEED, sigma_u=0.2, sigma_q=0.001, sigma_v=0.01, u_max=8.0, fall_height=0.16, kick_step=10), kick_y(shape, 0.3)),
    }
