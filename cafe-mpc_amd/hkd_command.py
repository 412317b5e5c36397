"""hkd_command_lcmt rows of an HKD-MPC handle (include/hsddp_hkd.h): the numpy specification and a decoder.

`pack_rows` builds the rows from what `Solver.field` returns, on any backend (the CPU checker included): it is the specification of
HKDMPCSolver::update_foot_placement + publish_mpc_cmd (HKDMPC/HKDMPC.cpp:207-297) that the device export (k_pack_hkd) matches bit for bit.
"""
import numpy as np

from ._abi import HKD_CMD_WORDS, HKD_MAX_STEPS, MODEL_HKD

# (name, first word, words, dtype, shape) in declaration order of lcmtypes/hkd_command_lcmt.lcm
LAYOUT = (("N_mpcsteps", 0, 1, np.int32, ()),
          ("mpc_times", 1, 20, np.float64, (10,)),
          ("hkd_controls", 21, 240, np.float32, (10, 24)),
          ("des_body_state", 261, 120, np.float32, (10, 12)),
          ("contacts", 381, 40, np.int32, (10, 4)),
          ("statusTimes", 421, 80, np.float64, (10, 4)),
          ("foot_placement", 501, 12, np.float32, (12,)),
          ("feedback", 513, 1440, np.float32, (10, 12, 12)),
          ("solve_time", 1953, 1, np.float32, ()))
OFFSETS = {name: off for name, off, _, _, _ in LAYOUT}


def step_map(horizons, n_steps):
    """Knot k of the message -> (phase, knot): the walk of publish_mpc_cmd (`if (s >= horizon) { s = 0; i++; }`).  None if the window is short."""
    out, s, i = [], 0, 0
    for _ in range(n_steps):
        if s >= horizons[i]:
            s = 0; i += 1
        if i >= len(horizons):
            return None
        out.append((i, s)); s += 1
    return out


def foothold_phases(contacts):
    """Leg l -> the phase whose first state holds its next foothold, or -1 (update_foot_placement: first 0 -> 1 boundary, i <= 4)."""
    fh = [-1] * 4
    for i in range(len(contacts) - 1):
        for l in range(4):
            if fh[l] < 0 and contacts[i][l] == 0 and contacts[i + 1][l] == 1:
                fh[l] = i + 1
        if i >= 4:
            break
    return fh


def _words(a, dtype):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype)).view(np.uint32)


def pack_rows(solver, b0=0, nb=None, n_steps=9, mpc_time=0.0, dt=0.01, status_times=None, pf=None):
    """uint32 [nb, HKD_CMD_WORDS]: the messages of problems b0 .. b0+nb-1 of `solver` (an HKD window), from its fields."""
    nb = solver.batch - b0 if nb is None else nb
    descs = [p["desc"] for p in solver.phases]
    if any(d.model != MODEL_HKD for d in descs) or not 1 <= n_steps <= HKD_MAX_STEPS:
        raise ValueError("an HKD window and 1 <= n_steps <= 10 are needed")
    walk = step_map([d.horizon for d in descs], n_steps)
    if walk is None:
        raise ValueError(f"the window has fewer than {n_steps} control knots")
    fields = {}

    def fld(i, name):
        if (i, name) not in fields:
            fields[(i, name)] = solver.field(i, name, b0=b0, nb=nb)
        return fields[(i, name)]

    rows = np.zeros((nb, HKD_CMD_WORDS), dtype=np.uint32)
    o = OFFSETS
    rows[:, 0] = n_steps
    rows[:, o["mpc_times"]:o["mpc_times"] + 2 * n_steps] = _words([mpc_time + k * dt for k in range(n_steps)], np.float64)
    st = None if status_times is None else np.asarray(status_times, dtype=np.float64)
    for k, (i, s) in enumerate(walk):
        rows[:, o["hkd_controls"] + 24 * k:o["hkd_controls"] + 24 * (k + 1)] = _words(fld(i, "UBAR")[:, s, :24], np.float32)
        rows[:, o["des_body_state"] + 12 * k:o["des_body_state"] + 12 * (k + 1)] = _words(fld(i, "XBAR")[:, s, :12], np.float32)
        rows[:, o["contacts"] + 4 * k:o["contacts"] + 4 * (k + 1)] = _words(list(descs[i].contact), np.int32)
        if st is not None:
            rows[:, o["statusTimes"] + 8 * k:o["statusTimes"] + 8 * (k + 1)] = _words(st[i], np.float64)
        fb = fld(i, "K")[:, s, :12, :12]            # K(m, n), m, n < 12, row-major
        rows[:, o["feedback"] + 144 * k:o["feedback"] + 144 * (k + 1)] = _words(fb.reshape(nb, 144), np.float32)
    pfi = np.zeros((nb, 12), dtype=np.float32) if pf is None else np.broadcast_to(np.asarray(pf, dtype=np.float32), (nb, 12)).copy()
    for l, f in enumerate(foothold_phases([list(d.contact) for d in descs])):
        if f >= 0:
            pfi[:, 3 * l:3 * l + 3] = fld(f, "XBAR")[:, 0, 12 + 3 * l:15 + 3 * l].astype(np.float32)
    rows[:, o["foot_placement"]:o["foot_placement"] + 12] = pfi.view(np.uint32)
    rows[:, o["solve_time"]] = np.float32(solver.solve_time_ms()).view(np.uint32)
    return rows


def decode(raw):
    """Decode one row (HKD_CMD_WORDS words) or a batch of rows into the hkd_command_lcmt fields (a leading batch axis on every field)."""
    raw = np.asarray(raw, dtype=np.uint32)
    out = {"raw": raw}
    for name, off, w, dt, shape in LAYOUT:
        seg = np.ascontiguousarray(raw[..., off:off + w]).view(dt)
        v = seg.reshape(raw.shape[:-1] + shape).copy()
        out[name] = v[()] if v.ndim == 0 else v
    if raw.ndim == 1:
        out["N_mpcsteps"] = int(out["N_mpcsteps"]); out["solve_time"] = float(out["solve_time"])
    return out
