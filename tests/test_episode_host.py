"""CPU tests of the MPC episodes (include/hsddp_episode.h): the ctypes mirror, the seed schedule, the phase table of the fixture, and the two
programs of cafe-mpc_amd/csrc/episode.hpp compiled for the host by tests/_emu/episode_emu.cpp - the pending reset map against the oracle's
rollout, the commit against episode.fold_rows.  Real HIP execution: tests/test_episode_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc
import episode_common as ec

ep = pkg.episode


def test_episode_abi_mirror_matches_the_header(tmp_path):
    """Every prototype of include/hsddp_episode.h is in EPISODE_EXPORTS and in no other list; hsddp_episode_row_t field for field."""
    src = open(os.path.join(ROOT, "include", "hsddp_episode.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = set(re.findall(r"\b(hsddp_[a-z_]+)\s*\(", code))
    A = pkg._abi
    assert protos == set(A.EPISODE_EXPORTS) and len(protos) == 9
    for other in (A.EXPORTS, A.ENSEMBLE_EXPORTS, A.HKD_EXPORTS, A.REFS_EXPORTS, A.SIM_EXPORTS, A.MC_EXPORTS, A.GRF_EXPORTS):
        assert not protos & set(other)
    body = re.search(r"typedef struct hsddp_episode_row \{(.*?)\} hsddp_episode_row_t;", code, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), ty) for n in names.split(",")]
    Row = A.EpisodeRow
    assert [(n, {"double": ctypes.c_double, "int": ctypes.c_int}[t]) for n, t in fields] == list(Row._fields_)
    assert A.EPISODE_ROW_DTYPE.itemsize == ctypes.sizeof(Row) == 96 and A.EPISODE_ROW_DTYPE.names == tuple(n for n, _ in Row._fields_)
    names = [n for n, _ in Row._fields_]
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp_episode.h"\nint main(void){ printf("%zu", sizeof(hsddp_episode_row_t));\n'
                    + "".join(f'printf(" %zu", offsetof(hsddp_episode_row_t, {n}));\n' for n in names) + 'printf("\\n"); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [ctypes.sizeof(Row)] + [getattr(Row, n).offset for n in names]
    assert [A.EPISODE_ROW_DTYPE.fields[n][1] for n in names] == got[1:]

    class Fake:      # bind_episode refuses a library that lacks a symbol
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.MC_EXPORTS + A.GRF_EXPORTS + A.EPISODE_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_episode(lib)
    setattr(lib, A.EPISODE_EXPORTS[-1], Fake())
    A.bind_episode(lib)
    assert lib.hsddp_episode_sim.restype is ctypes.c_void_p and len(lib.hsddp_episode_advance.argtypes) == 4


def test_tick_seed_is_the_seed_then_the_raw_splitmix_outputs():
    M = (1 << 64) - 1
    for seed in (0, 7, 20241222, M, -3):
        assert ep.tick_seed(seed, 0) == seed & M
        rng = pkg.problems.SplitMix64(seed)
        vals = [ep.tick_seed(seed, 0)]
        for t in (1, 2, 3):
            u = rng.next()      # advances the state; the raw output is the mixed state in front of the shift that makes the double
            z = rng.s
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            assert ep.tick_seed(seed, t) == z and (z >> 11) * (1.0 / 9007199254740992.0) == u
            vals.append(z)
        assert len(set(vals)) == 4


def test_bound_fixture_ends_tick_one_on_the_flight_touchdown():
    """The case the episode exists for: from window 11, tick index 1 runs in window 12, whose leading phase is the flight phase with exactly n_exec
    knots left and a touchdown behind it."""
    pd, phases, cfg, _, _, n_exec = ec.bound_problem(pkg)
    assert n_exec == 2
    pd.update()
    ph12, info = pd.describe(ubar_mode="zero")
    assert info["horizons"] == [2, 10, 10, 3] and info["contacts"][0] == [0, 0, 0, 0] and info["has_td"][0]
    d = ph12[0]["desc"]
    assert any(d.contact[l] == 0 and d.next_contact[l] == 1 for l in range(4))
    smap = sc.step_map(phases, n_exec)
    assert smap[2].sum() == 0 and phases[0]["desc"].horizon > n_exec      # window 11 itself does not end on a phase boundary


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return ec.build_emu(tmp_path_factory.mktemp("episode_emu"))


def test_impact_program_on_the_host_matches_the_oracle(emu, oracle_lib):
    """The state at the end of phase 0 and, behind the reset map, at knot 0 of phase 1 of the oracle's single-shooting rollout: the program applied to
    the former gives the latter, hands it to the solver, and leaves a frozen problem alone."""
    phases = pkg.problems.wb_trot_problem(schedule=((0, 1, 1, 0), (1, 0, 0, 1)), horizons=(8, 8), last_next=(0, 1, 1, 0))
    x0 = pkg.problems.wb_ensemble_x0(4, 20241220)
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(x0); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3))
    xs = so.field(0, "XBAR")[:, 0] + pkg.problems.perturbed_states(np.zeros((4, 36)), 2, 0.02, 0.2, seed=5)[:, 1]
    so.set_initial_condition(np.ascontiguousarray(xs)); so.hybrid_rollout(0.0, pkg.mhpc_ddp_setting(MS=0))
    before = np.ascontiguousarray(so.field(0, "X")[:, 8]); after = so.field(1, "X")[:, 0]
    assert np.array_equal(before[:, :18], after[:, :18]) and np.abs(before[:, 18:] - after[:, 18:]).max() > 1e-3      # a real impact
    d = phases[0]["desc"]
    td = [1 if (d.contact[l] == 0 and d.next_contact[l] == 1) else 0 for l in range(4)]
    assert td == [1, 0, 0, 1]
    rows = ep.empty_rows(4); rows["end_reason"][2] = 1
    state = before.copy(); hand = np.full((4, 36), -7.0)
    ec.emu_impact(emu, td, d.BG_alpha, rows, state, hand)
    live = [0, 1, 3]
    sc.close("impact state", state[live], after[live])
    assert np.array_equal(hand[live], state[live]) and np.array_equal(state[live, :18], before[live, :18])
    assert np.array_equal(state[2], before[2]) and (hand[2] == -7.0).all()
    so.close()


def hand_made_tick(rng, per_problem):
    """3 problems, n_exec = 2, tick 1 of 3; two phases (h = 3, 2), the tick's steps are the last knot of phase 0 and the first of phase 1.  Problem 0
    stays alive, problem 1 falls at step 1, problem 2 is frozen already."""
    B, n, T = 3, 2, 3
    hor = [3, 2]
    smap = np.array([[0, 1], [2, 0], [1, 0]], dtype=np.int32)
    q = rng.uniform(0.0, 5.0, (2, 36)); r = rng.uniform(0.0, 2.0, (2, 12))
    pb = [0, 3] if per_problem else [0, 0]
    rref = [rng.normal(size=((B if pb[p] else 1) * (hor[p] + 1), 80)) for p in range(2)]
    t = dict(B=B, n=n, T=T, hor=hor, smap=smap, q=q, r=r, pb=pb, rref=rref)
    t["X"] = rng.normal(size=(B, n + 1, 36)); t["U"] = rng.normal(size=(B, n, 12)); t["Y"] = rng.normal(size=(B, n, 12)); t["fin"] = t["X"][:, -1].copy()
    t["sim"] = np.column_stack([rng.uniform(0, 1, B), rng.uniform(0, 3, B), rng.uniform(0.1, 0.3, B), rng.uniform(5, 20, B), [-1.0, -1.0, 0.0]])
    t["extra"] = np.array([[-1.0, 3.0], [1.0, 5.0], [0.0, 9.0]])
    t["grf"] = np.column_stack([rng.uniform(-5, 50, B), rng.uniform(-5, 20, B), rng.uniform(50, 200, B), [1.0, -1.0, 0.0], [2.0, 0.0, 4.0]])
    t["status"] = np.array([1, 0, 1], dtype=np.int32)
    rows = ep.empty_rows(B)
    for f in ("dev_q", "dev_v", "min_height", "max_torque", "min_fz", "min_cone", "max_fz", "track_cost"):
        rows[f] = rng.uniform(0.2, 2.0, B)
    rows["n_sat"] = [1, 2, 3]; rows["n_slip"] = [0, 1, 2]; rows["steps"] = [2, 2, 2]; rows["bad_solves"] = [0, 1, 0]
    rows["end_reason"][2] = 1; rows["end_step"][2] = 1
    t["rows"] = rows
    return t


def tick_refs(t):
    """xr [B, n, 36], ur [B, n, 12] of the hand-made tick from its records, as the header states the row of a problem."""
    xr = np.zeros((t["B"], t["n"], 36)); ur = np.zeros((t["B"], t["n"], 12))
    for b in range(t["B"]):
        for s in range(t["n"]):
            p, k = t["smap"][0][s], t["smap"][1][s]
            rec = t["rref"][p][b * t["pb"][p] + k]
            xr[b, s] = rec[:36]; ur[b, s] = rec[36:48]
    return xr, ur


@pytest.mark.parametrize("per_problem", [False, True])
@pytest.mark.parametrize("handoff", [1, 0])
def test_commit_program_on_the_host_matches_fold_rows(emu, per_problem, handoff):
    t = hand_made_tick(np.random.default_rng(11 + per_problem), per_problem)
    B, n, T = t["B"], t["n"], t["T"]
    rows = t["rows"].copy(); state = np.full((B, 36), 3.0); x0 = np.full((B, 36), -7.0)
    logX = np.full((B, T * n + 1, 36), 9.0); logU = np.full((B, T * n, 12), 9.0); logY = np.full((B, T * n, 12), 9.0)
    ec.emu_commit(emu, t["hor"], t["q"], t["r"], t["rref"], t["pb"], t["status"], 1, T, handoff, t["smap"], t["X"], t["U"], t["Y"], t["fin"], t["sim"], t["extra"], t["grf"],
                  rows, state, x0, logX, logU, logY)
    xr, ur = tick_refs(t)
    q = t["q"][t["smap"][0]]; r = t["r"][t["smap"][0]]
    want = ep.fold_rows(t["rows"], 1, ec.sim_rows_struct(pkg, t["sim"]), t["X"], t["U"], q, r, xr, ur, extra=ec.extra_struct(pkg, t["extra"]), grf=ec.grf_struct(pkg, t["grf"]),
                        status=t["status"])
    for f in rows.dtype.names:
        if f != "track_cost":
            assert np.array_equal(rows[f], want[f]), f
    rel = np.abs(rows["track_cost"] - want["track_cost"]) / np.abs(want["track_cost"])
    print(f"[episode] track_cost host build vs fold_rows: rel {rel.max():.3e}")
    assert rel.max() <= 1e-12
    # by value: problem 0 goes on, problem 1 fell at step 1 of tick 1 = global step 3, problem 2 was frozen and is untouched
    assert list(rows["end_reason"]) == [0, 2, 1] and list(rows["end_step"]) == [-1, 3, 1] and list(rows["steps"]) == [4, 4, 2]
    assert list(rows["bad_solves"]) == [1, 1, 0] and list(rows["n_sat"]) == [4, 7, 3] and list(rows["first_slip"]) == [3, -1, -1] and list(rows["n_slip"]) == [2, 1, 2]
    assert rows[2:].tobytes() == t["rows"][2:].tobytes()
    assert rows["track_cost"][0] > t["rows"]["track_cost"][0]
    for b in (0, 1):
        assert np.array_equal(logX[b, 2:5], t["X"][b]) and np.array_equal(logU[b, 2:4], t["U"][b]) and np.array_equal(logY[b, 2:4], t["Y"][b])
        assert (logX[b, :2] == 9.0).all() and (logX[b, 5:] == 9.0).all() and (logU[b, :2] == 9.0).all() and (logU[b, 4:] == 9.0).all()
        assert np.array_equal(state[b], t["fin"][b])
    assert (logX[2] == 9.0).all() and (logU[2] == 9.0).all() and (logY[2] == 9.0).all() and (state[2] == 3.0).all()
    # the hand-off: only a problem still alive, and only when no reset map is pending (the impact program hands over then)
    assert (np.array_equal(x0[0], t["fin"][0]) if handoff else (x0[0] == -7.0).all()) and (x0[1:] == -7.0).all()


def test_commit_program_without_extras_records_or_log(emu):
    """A plain walk: no extras (nothing falls), no force records, no log; divergence ends the episode with reason 1."""
    t = hand_made_tick(np.random.default_rng(3), False)
    B, n, T = t["B"], t["n"], t["T"]
    t["sim"][1, 4] = 0.0
    rows = t["rows"].copy(); state = np.zeros((B, 36)); x0 = np.zeros((B, 36))
    ec.emu_commit(emu, t["hor"], t["q"], t["r"], t["rref"], t["pb"], t["status"], 1, T, 1, t["smap"], t["X"], t["U"], None, t["fin"], t["sim"], None, None,
                  rows, state, x0, None, None, None)
    xr, ur = tick_refs(t)
    want = ep.fold_rows(t["rows"], 1, ec.sim_rows_struct(pkg, t["sim"]), t["X"], t["U"], t["q"][t["smap"][0]], t["r"][t["smap"][0]], xr, ur, status=t["status"])
    for f in rows.dtype.names:
        if f != "track_cost":
            assert np.array_equal(rows[f], want[f]), f
    assert np.allclose(rows["track_cost"], want["track_cost"], rtol=1e-12, atol=0)
    assert list(rows["end_reason"]) == [0, 1, 1] and list(rows["end_step"]) == [-1, 2, 1]
    for f in ("min_fz", "min_cone", "max_fz", "first_slip", "n_slip", "n_sat"):
        assert np.array_equal(rows[f], t["rows"][f]), f


def test_fold_rows_fell_wins_only_when_not_later_than_the_divergence():
    rows = ep.empty_rows(3)
    sim = np.zeros(3, dtype=pkg._abi.SIM_ROW_DTYPE); sim["first_bad"] = [1, 1, 0]
    ex = np.zeros(3, dtype=pkg._abi.MC_EXTRA_DTYPE); ex["first_fall"] = [1, 0, 1]
    z = np.zeros((3, 3, 36)); u = np.zeros((3, 2, 12))
    out = ep.fold_rows(rows, 2, sim, z, u, np.ones((2, 36)), np.ones((2, 12)), z[:, :2], u, extra=ex)
    assert list(out["end_reason"]) == [2, 2, 1] and list(out["end_step"]) == [5, 4, 4] and (out["track_cost"] == 0).all()


def test_multiphase_ddp_header_compiles_with_episode(tmp_path):
    """The C++ mirror: hsddp::Episode compiles, and so does the harness tests/cpp/episode_loop.cpp (linked and run in tests/test_episode_gpu.py)."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0) {\n'
                   '    hsddp::Episode e(s.handle(), 2, 2, 8, true); e.reset(x0); e.set_grf(0.6); e.advance();\n'
                   '    hsddp_mc_dist_t d = hsddp::default_disturbance(); e.advance(&d, x0);\n'
                   '    auto r = e.rows(); (void)r[0].end_reason; auto l = e.log(); (void)l.Y.size(); (void)e.state(); (void)e.last_error();\n'
                   '    int t, a, i; e.status(&t, &a, &i);\n'
                   '}\n')
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host")]
    subprocess.check_call(["g++", "-std=c++17", "-c"] + inc + [str(src), "-o", str(tmp_path / "w.o")])
    subprocess.check_call(["g++", "-std=c++17", "-c"] + inc + [os.path.join(ROOT, "tests", "cpp", "episode_loop.cpp"), "-o", str(tmp_path / "l.o")])


def test_reference_episode_applies_the_pending_impact_once(emu, oracle_lib, tmp_path):
    """The loop composed of the oracle solver and the host builds of walk, commit and reset map, three ticks from window 11: tick index 1 ends on the
    flight phase's touchdown, so the reset map runs exactly once; the log is continuous across the tick boundaries except there, where only the
    velocities jump."""
    B, T = 2, 3
    out = ec.reference_episode(pkg, oracle_lib, ec.build_sim_emu(tmp_path), emu, B, T)
    n = out["n_exec"]
    assert out["n_impacts"] == 1 and out["impact_ticks"] == [1]
    assert (out["rows"]["steps"] == T * n).all() and (out["rows"]["end_reason"] == 0).all() and (out["rows"]["track_cost"] > 0).all()
    for t in range(T - 1):
        a, b = out["finals"][t], out["starts"][t + 1]
        if t == 1:
            assert np.array_equal(a[:, :18], b[:, :18]) and np.abs(a[:, 18:] - b[:, 18:]).max() > 1e-3
        else:
            assert np.array_equal(a, b)
        assert np.array_equal(out["X"][:, (t + 1) * n], b)      # the next tick's entry 0 is what the log keeps at the boundary
    assert np.array_equal(out["X"][:, T * n], out["finals"][-1]) and np.array_equal(out["state"], out["finals"][-1])
    # forward Euler in the positions at every logged step, the boundaries included: q[k + 1] = q[k] + dt v[k] with the velocity the log keeps at k
    X = out["X"]
    assert np.abs(np.diff(X[:, :, :18], axis=1) - 0.01 * X[:, :-1, 18:]).max() <= 1e-13 * max(1.0, np.abs(X).max())
