"""Shared by tests/test_episode_host.py and tests/test_episode_gpu.py: the bound-gait fixture of the MPC episodes (include/hsddp_episode.h), the
raw-row conversions between the walk's device layout and the ctypes mirrors, and the host build of the commit / pending reset map
(tests/_emu/episode_emu.cpp) behind numpy arguments."""
import ctypes
import os

import numpy as np

import sim_common
import walk_ref
from conftest import ROOT

TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")
START_WINDOW = 11      # the builder advanced this many MPC steps on the host: two ticks later the flight phase's touchdown falls on a tick boundary


def bound_problem(pkg, n_updates=START_WINDOW):
    """(pd, phases, cfg, opt0, opt_rt, n_exec) of the bound gait fixture with the builder advanced n_updates MPC steps on the host."""
    import importlib
    builder = importlib.import_module(pkg.__name__ + ".builder")
    cfg = builder.load_mhpc_config(TREE + "/MHPC/settings/mhpc_config.info")
    pd = builder.MHPCProblemData(builder.QuadReference(TREE + "/Reference/Data/bound/quad_reference.csv"), cfg,
                                 builder.load_cost_weights(TREE + "/" + cfg["costFile"]), builder.load_constraint_params(TREE + "/" + cfg["constraintParamFile"]))
    for _ in range(n_updates):
        pd.update()
    phases, _ = pd.describe(ubar_mode="zero")
    opt0 = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info")
    opt_rt = builder.load_ddp_setting(TREE + "/MHPC/settings/ddp_setting.info")
    opt_rt.max_AL_iter, opt_rt.max_DDP_iter = opt_rt.max_AL_iter_runtime, opt_rt.max_DDP_iter_runtime
    return pd, phases, cfg, opt0, opt_rt, int(round(float(cfg["dt_mpc"]) / cfg["dt_wb"]))


def build_host(tmpdir, source, name):
    """A host build of a kernel program: tests/_emu/<source> compiled with g++ into tmpdir, as tests/test_sim_host.py compiles sim_emu.cpp."""
    return walk_ref.build_so(tmpdir, source, name)


def build_emu(tmpdir):
    lib = build_host(tmpdir, "episode_emu.cpp", "libhsddp_episode_emu.so")
    assert lib.episode_emu_row_bytes() == 96
    return lib


def sim_rows_struct(pkg, raw):
    """[B, 5] doubles as the walk leaves them -> SIM_ROW_DTYPE."""
    r = np.zeros(raw.shape[0], dtype=pkg._abi.SIM_ROW_DTYPE)
    for i, f in enumerate(("dev_q", "dev_v", "min_height", "max_torque", "first_bad")):
        r[f] = raw[:, i]
    return r


def extra_struct(pkg, raw):
    r = np.zeros(raw.shape[0], dtype=pkg._abi.MC_EXTRA_DTYPE)
    r["first_fall"] = raw[:, 0]; r["n_sat"] = raw[:, 1]
    return r


def grf_struct(pkg, raw):
    r = np.zeros(raw.shape[0], dtype=pkg._abi.GRF_ROW_DTYPE)
    for i, f in enumerate(("min_fz", "min_cone", "max_fz", "first_slip", "n_slip")):
        r[f] = raw[:, i]
    return r


def vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def emu_commit(lib, horizons, q, r, rref, ref_pb, status, tick, max_ticks, handoff, smap, simX, simU, simY, fin, sim_rows, extra, grf_rows, rows, state, x0, logX, logU, logY):
    """The host build of k_episode_commit over the batch; rows, state, x0 and the logs are updated in place.  q [nph, 36], r [nph, 12]; rref: one
    array of 80-double records per phase; the raw rows are [B, 5] / [B, 2] / [B, 5] doubles."""
    nph, B, n = len(horizons), simU.shape[0], simU.shape[1]
    hor = np.ascontiguousarray(horizons, dtype=np.int32); pb = np.ascontiguousarray(ref_pb, dtype=np.int32); st = np.ascontiguousarray(status, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.float64); r = np.ascontiguousarray(r, dtype=np.float64)
    ptrs = (ctypes.c_void_p * nph)(*[a.ctypes.data for a in rref])
    rc = lib.episode_emu_commit(nph, vp(hor), vp(q), vp(r), ptrs, vp(pb), B, vp(st), n, tick, max_ticks, handoff, vp(np.ascontiguousarray(smap, dtype=np.int32)),
                                vp(simX), vp(simU), vp(simY), vp(fin), vp(sim_rows), vp(extra), vp(grf_rows), vp(rows), vp(state), vp(x0), vp(logX), vp(logU), vp(logY))
    assert rc == 0
    return rows


def emu_impact(lib, td, bg_alpha, rows, state, x0, psi_dyn=3.1415):
    """The host build of k_episode_impact on state [B, 36] (in place) and the hand-off destination x0."""
    t = np.ascontiguousarray(td, dtype=np.int32)
    rc = lib.episode_emu_impact(vp(t), ctypes.c_double(bg_alpha), ctypes.c_double(psi_dyn), state.shape[0], vp(rows), vp(state), vp(x0))
    assert rc == 0


def pending_phase(phases, n_exec):
    """The phase whose reset map lies behind step n_exec - 1 of the window (the tick ends exactly on its touchdown), else -1."""
    n = 0
    for i, p in enumerate(phases):
        d = p["desc"]
        if d.model != 0:
            break
        if n + d.horizon >= n_exec:
            td = any(d.contact[l] == 0 and d.next_contact[l] == 1 for l in range(4))
            return i if (td and n + d.horizon == n_exec) else -1
        n += d.horizon
    return -1


def start_states(pkg, phases, B, seed=20241222):
    """B states around the window's first reference state (sigma 0.002 / 0.02; problem 0 starts on it)."""
    x = np.repeat(phases[0]["Xbar"][:1], B, axis=0)
    out = pkg.problems.perturbed_states(x, 2, 0.002, 0.02, seed=seed)[:, 1]
    out[0] = x[0]
    return np.ascontiguousarray(out)


def shift(pkg, solver, phases, pd):
    """The window of `solver` moved by one MPC step in place; returns the new phases."""
    import importlib
    builder = importlib.import_module(pkg.__name__ + ".builder")
    m = pd.update()
    phases, _ = builder.shift_solver_in_place(solver, phases, pd, m, ubar_mode="zero")
    return phases


def build_sim_emu(tmpdir):
    """The host build of the plain walk (tests/_emu/sim_emu.cpp)."""
    return build_host(tmpdir, "sim_emu.cpp", "libhsddp_sim_emu.so")


def emu_walk(lib, so, phases, b, x0, smap):
    """The host build of the walk on problem b of a solved handle from the state x0 [36]: (final [36], row [5], X [n + 1, 36], U [n, 12])."""
    nph = sum(1 for p in phases if p["desc"].model == 0)
    D = [p["desc"] for p in phases[:nph]]
    hor = np.array([d.horizon for d in D], dtype=np.int32); dt = np.array([d.dt for d in D]); al = np.array([d.BG_alpha for d in D])
    ct = np.array([[d.contact[l] for l in range(4)] for d in D], dtype=np.int32)
    td = np.array([[1 if (d.contact[l] == 0 and d.next_contact[l] == 1) else 0 for l in range(4)] for d in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]      # column-major 12 x 36 per knot
    ptrs = lambda arrs: (ctypes.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n = smap.shape[1]
    x0 = np.ascontiguousarray(x0.reshape(1, 36))
    xf = np.zeros((1, 36)); rows = np.zeros((1, 5)); X = np.zeros((1, n + 1, 36)); U = np.zeros((1, n, 12))
    rc = lib.sim_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), ctypes.c_double(3.1415), vp(np.ascontiguousarray(smap)), n, 1,
                         vp(x0), vp(xf), vp(rows), vp(X), vp(U))
    assert rc == 0
    return xf[0], rows[0], X[0], U[0]


def shared_rref(phases):
    """Per whole-body phase the 80-double reference records of its knots (xr | ur | the rest unused by the commit), q [nph, 36], r [nph, 12]."""
    rref, q, r, hor = [], [], [], []
    for p in phases:
        d = p["desc"]
        if d.model != 0:
            break
        h = d.horizon
        rec = np.zeros((h + 1, 80))
        rec[:, :36] = np.ctypeslib.as_array(d.xr, shape=(h + 1, 36)); rec[:, 36:48] = np.ctypeslib.as_array(d.ur, shape=(h + 1, 12))
        rref.append(rec); q.append([d.q[i] for i in range(36)]); r.append([d.r[j] for j in range(12)]); hor.append(h)
    return hor, np.array(q), np.array(r), rref


def reference_episode(pkg, oracle_lib, sim_lib, epi_lib, B, T):
    """The loop composed of what exists, on the bound gait fixture from window 11 (plain walk): the oracle solver (solve / reconfigure), the host
    build of the walk, the host builds of the commit and of the pending reset map.  Returns a dict: rows, state, logs X / U, n_impacts, and per tick
    the trajectory's last entry (`finals`) and the next tick's first (`starts`) - the pair a tick boundary joins."""
    pd, phases, cfg, opt0, opt_rt, n = bound_problem(pkg)
    opt0.max_AL_iter, opt0.max_DDP_iter = 3, 4
    x0 = start_states(pkg, phases, B)
    so = pkg.Solver(oracle_lib, phases, batch=B)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(x0); so.solve(opt0)
    rows = pkg.episode.empty_rows(B); state = x0.copy(); ic = x0.copy()
    logX = np.zeros((B, T * n + 1, 36)); logU = np.zeros((B, T * n, 12))
    finals, starts, n_imp, impact_ticks = [], [], 0, []
    for t in range(T):
        smap, pend = sim_common.step_map(phases, n), pending_phase(phases, n)
        walks = [emu_walk(sim_lib, so, phases, b, state[b], smap) for b in range(B)]
        fin = np.stack([w[0] for w in walks]); srows = np.stack([w[1] for w in walks]); X = np.stack([w[2] for w in walks]); U = np.stack([w[3] for w in walks])
        starts.append(X[:, 0].copy()); finals.append(X[:, -1].copy())
        hor, q, r, rref = shared_rref(phases)
        emu_commit(epi_lib, hor, q, r, rref, [0] * len(hor), so.info_arrays()["status"], t, T, 0 if pend >= 0 else 1, smap, X, U, None, fin, srows, None, None,
                   rows, state, ic, logX, logU, None)
        if pend >= 0:
            d = phases[pend]["desc"]
            emu_impact(epi_lib, [1 if (d.contact[l] == 0 and d.next_contact[l] == 1) else 0 for l in range(4)], d.BG_alpha, rows, state, ic)
            n_imp += 1; impact_ticks.append(t)
        so.set_initial_condition(ic)
        phases = shift(pkg, so, phases, pd)
        so.solve(opt_rt)
    so.close()
    return dict(rows=rows, state=state, X=logX, U=logU, n_impacts=n_imp, impact_ticks=impact_ticks, finals=finals, starts=starts, n_exec=n)

