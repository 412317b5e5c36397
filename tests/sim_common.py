"""Shared by tests/test_sim_host.py and tests/test_sim_gpu.py: reference values of a closed-loop simulation window from the oracle's existing
entry points, and the comparison against them.

Reference of sample r: on an oracle handle that has solved the problem, set_initial_condition(x0[:, r]) and hybrid_rollout(0.0, MS = 0) - the
single-shooting chain evaluates u = Ubar + K (X - Xbar) from that state and leaves Xbar, Ubar, K alone - then X and U of the window's knots.
Tolerance: 1e-8 x the field's scale, the plain rollout tolerance of parity_common (the fp64 oracle sits <= 1e-12 from its long-double build on
these windows, so no arbiter is involved)."""
import numpy as np

RTOL = 1e-8


def step_map(phases, n_steps):
    """step -> (phase, knot, reset map applied behind the step) over the leading whole-body control knots, as hsddp_sim_create lays it out."""
    out = []
    for i, p in enumerate(phases):
        d = p["desc"]
        if d.model != 0:
            break
        td = any(d.contact[l] == 0 and d.next_contact[l] == 1 for l in range(4))
        for k in range(d.horizon):
            out.append([i, k, 1 if (td and k == d.horizon - 1) else 0])
    assert len(out) >= n_steps
    out = out[:n_steps]
    out[-1][2] = 0          # the window ends here: the final state is the one before any reset map
    return np.ascontiguousarray(np.array(out, dtype=np.int32).T)


def window(fields_by_phase, smap, final):
    """Rows of a per-phase field [nb, count, w] at the window's knots; final: also the row behind the last step."""
    rows = [fields_by_phase[p][:, k] for p, k in zip(smap[0], smap[1])]
    if final:
        rows.append(fields_by_phase[smap[0][-1]][:, smap[1][-1] + 1])
    return np.stack(rows, axis=1)


def oracle_reference(so, opt_ss, x0, smap):
    """so: a solved oracle handle of batch B; x0: [B, R, 36].  Returns X [B, R, n+1, 36], U [B, R, n, 12] of the window and XBAR [B, n+1, 36]."""
    nph = len(so.phases)
    B, R = x0.shape[:2]
    xbar = window([so.field(i, "XBAR") for i in range(nph)], smap, True)
    X = np.zeros((B, R, smap.shape[1] + 1, 36)); U = np.zeros((B, R, smap.shape[1], 12))
    for r in range(R):
        so.set_initial_condition(np.ascontiguousarray(x0[:, r]))
        so.hybrid_rollout(0.0, opt_ss)
        X[:, r] = window([so.field(i, "X") for i in range(nph)], smap, True)
        U[:, r] = window([so.field(i, "U") for i in range(nph)], smap, False)
    assert np.array_equal(xbar, window([so.field(i, "XBAR") for i in range(nph)], smap, True))      # the policy was not touched
    return X, U, xbar


def rows_of(X, U, xbar):
    """The per-sample summary recomputed from trajectories: dev_q, dev_v, min_height, max_torque."""
    d = np.abs(X - xbar[:, None])
    return dict(dev_q=d[..., :18].max(axis=(2, 3)), dev_v=d[..., 18:].max(axis=(2, 3)), min_height=X[..., 2].min(axis=2), max_torque=np.abs(U).max(axis=(2, 3)))


def close(tag, a, ref, scale=None):
    """|a - ref| <= RTOL x max(1, |ref|max), printed before it is asserted."""
    sc = max(1.0, float(np.abs(ref).max())) if scale is None else scale
    err = float(np.abs(a - ref).max())
    print(f"[sim] {tag}: |diff| = {err:.3e}, scale {sc:.3e}, bound {RTOL * sc:.3e}")
    assert np.isfinite(a).all(), tag
    assert err <= RTOL * sc, f"{tag}: |diff| = {err:.3e} > {RTOL * sc:.3e} (scale {sc:.3e})"


def compare_window(tag, res, X, U, xbar):
    """res: dict with rows (structured), x_final and optionally X, U of the backend under test against the oracle's window."""
    if "X" in res:
        close(tag + " X", res["X"], X); close(tag + " U", res["U"], U)
    close(tag + " x_final", res["x_final"], X[:, :, -1])
    ref = rows_of(X, U, xbar)
    for f in ("dev_q", "dev_v", "min_height", "max_torque"):
        # relative to the summary's own largest value over the batch, without the floor of 1 the trajectories get: the deviations are maxima of
        # DIFFERENCES of states of order one, so an entry-by-entry relative bound would ask more of a small deviation than fp64 can give
        close(f"{tag} {f}", res["rows"][f], ref[f], scale=float(np.abs(ref[f]).max()))
    assert (res["rows"]["first_bad"] == -1).all(), tag
