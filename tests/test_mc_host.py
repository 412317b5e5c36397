"""CPU tests of the disturbed closed-loop simulation (include/hsddp_mc.h): the ctypes mirror, the generator's numpy statement (sim.mc_normals),
the reference walk (tests/mc_common.py) against the oracle's rollout and against the figures recorded for the cases, and the disturbed program
itself (cafe-mpc_amd/csrc/wb_sim.hpp with the WbsMc policy) compiled for the host by tests/_emu/mc_emu.cpp.  Real HIP: tests/test_mc_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc
import mc_common as mc


def test_mc_abi_mirror_matches_the_header(tmp_path):
    """hsddp_mc_dist_t and hsddp_mc_extra_t against a compiled C probe, every prototype of include/hsddp_mc.h bound."""
    src = open(os.path.join(ROOT, "include", "hsddp_mc.h")).read()
    Dist, Extra = pkg._abi.McDist, pkg._abi.McExtra
    names = [n for n, _ in Dist._fields_]
    assert names == ["seed", "sigma_u", "sigma_q", "sigma_v", "u_max", "fall_height", "kick_step", "first_problem"]
    for n in names:      # every field of the mirror is declared in the header's struct
        body = re.search(r"typedef struct hsddp_mc_dist \{(.*?)\} hsddp_mc_dist_t;", src, re.S).group(1)
        assert re.search(r"\b%s\b" % n, body), n
    csrc = tmp_path / "sz.c"
    offs = ", ".join(f"offsetof(hsddp_mc_dist_t, {n})" for n in names)
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp_mc.h"\nint main(void){ size_t v[] = {sizeof(hsddp_mc_dist_t), ' + offs +
                    ', sizeof(hsddp_mc_extra_t), offsetof(hsddp_mc_extra_t, first_fall), offsetof(hsddp_mc_extra_t, n_sat)};\n'
                    'for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%zu ", v[i]); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    want = [ctypes.sizeof(Dist)] + [getattr(Dist, n).offset for n in names] + [ctypes.sizeof(Extra), Extra.first_fall.offset, Extra.n_sat.offset]
    assert got == want and ctypes.sizeof(Dist) == 56 and ctypes.sizeof(Extra) == 8
    assert pkg._abi.MC_EXTRA_DTYPE.itemsize == 8 and pkg._abi.MC_EXTRA_DTYPE.names == ("first_fall", "n_sat")
    protos = set(re.findall(r"\b(hsddp_mc_[a-z_]+)\s*\(", src))
    assert protos == set(pkg._abi.MC_EXPORTS) and len(protos) == 2
    assert len(pkg._abi.SIM_EXPORTS) == 7 and not set(pkg._abi.MC_EXPORTS) & set(pkg._abi.EXPORTS)

    class Fake:
        pass
    lib = Fake()
    for s in pkg._abi.SIM_EXPORTS + pkg._abi.MC_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        pkg._abi.bind_mc(lib)
    setattr(lib, pkg._abi.MC_EXPORTS[-1], Fake())
    pkg._abi.bind_mc(lib)
    assert len(lib.hsddp_mc_run.argtypes) == 6 and len(lib.hsddp_mc_get_extra.argtypes) == 4
    d = pkg.sim.Disturbance(seed=(1 << 64) - 3, sigma_u=0.5, u_max=7.0, kick_step=4, first_problem=9).to_c()
    assert (d.seed, d.sigma_u, d.sigma_q, d.u_max, d.kick_step, d.first_problem) == ((1 << 64) - 3, 0.5, 0.0, 7.0, 4, 9)


def test_mc_normals_are_the_stated_generator():
    """Seeded, a pure function of (seed, problem, sample, step); its uniforms are SplitMix64(seed) advanced to draw number n0."""
    f = pkg.sim.mc_normals
    a = f(11, 2, 3, 4)
    assert a.shape == (48,) and a.dtype == np.float64 and np.array_equal(a, f(11, 2, 3, 4))
    for other in (f(12, 2, 3, 4), f(11, 3, 3, 4), f(11, 2, 4, 4), f(11, 2, 3, 5)):
        assert not np.array_equal(a, other)
    for c in (0, 11, 12, 47):
        n0 = 2 * ((((2 * 65536) + 3) * 65536 + 4) * 48 + c)
        rng = pkg.problems.SplitMix64(11); rng.skip(n0)
        u1, u2 = rng.next(), rng.next()
        assert a[c] == np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2), c
    big = f(20241222, 1000000, 65535, 65535)      # the largest draw numbers of a million problems stay below 2^64
    assert np.isfinite(big).all() and 2 * ((((1000000 * 65536) + 65535) * 65536 + 65535) * 48 + 48) < 1 << 64
    with pytest.raises(ValueError):
        f(1, 0, 65536, 0)
    z = np.array([f(11, p, r, s) for p in range(3) for r in range(8) for s in range(100)])
    corr = np.corrcoef(z.T) - np.eye(48)
    print(f"[mc] normals: mean {z.mean():+.4f}, std {z.std():.4f}, largest correlation {np.abs(corr).max():.3f}")
    assert z.shape == (2400, 48) and abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.05 and np.abs(corr).max() < 0.1


@pytest.fixture(scope="module")
def solved_trot(oracle_lib):
    """The fixture of tests/test_sim_gpu.py: trot 4 x 12, four problems, 3 AL x 4 DDP iterations, eight samples around Xbar[0] (sigma 0.02 / 0.2)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    x0 = pkg.problems.wb_ensemble_x0(4, 20241222)
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(x0); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    return phases, so, xs, mc.policy_of(so)


def test_undisturbed_walk_is_the_oracle_rollout(oracle_lib, solved_trot):
    """What makes the walk a reference: with every switch off it reproduces hybrid_rollout(0, MS = 0) (recorded: 1.5e-13 on X and U)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    X, U, xbar = sc.oracle_reference(so, pkg.mhpc_ddp_setting(MS=0), xs, smap)
    w = mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs)
    ex, eu = np.abs(w["X"] - X).max(), np.abs(w["U"] - U).max()
    print(f"[mc] undisturbed walk against hybrid_rollout: X {ex:.2e}, U {eu:.2e}")
    assert ex < 1e-11 and eu < 1e-11      # round-off of the same arithmetic in another order of operations; the comparison bound is 1e-8
    assert np.array_equal(xbar, mc.xbar_window(pol, smap))
    assert (w["first_bad"] == -1).all() and (w["first_fall"] == -1).all() and (w["n_sat"] == 0).all()


@pytest.fixture(scope="module")
def walks(oracle_lib, solved_trot):
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    return {name: mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs, d, k) for name, (d, k) in mc.cases(pkg, xs.shape[:2]).items()}


def test_oracle_walk_gives_the_recorded_figures(walks):
    """The figures recorded for cases A - D with the generator as defined and seed 20241222: a change of the generator or of the walk shows here."""
    for name, w in walks.items():
        print(f"[mc] case {name}: n_sat {int(w['n_sat'].sum())} on {int((w['n_sat'] > 0).sum())} samples, falls {int((w['first_fall'] >= 0).sum())}, torque margin "
              f"{w['sat_margin'].min():.2e}, height margin {w['fall_margin'].min():.2e}, lowest {w['X'][..., 2].min():.3f}, max |u| {np.abs(w['U']).max():.2f}")
        assert (w["first_bad"] == -1).all() and np.isfinite(w["X"]).all()
        assert not ((w["sat_margin"] < mc.NEAR) | (w["fall_margin"] < mc.NEAR)).any()      # the reference alone leaves no sample out
    a, b, c, d = (walks[k] for k in "ABCD")
    assert a["n_sat"].sum() == 0 and abs(np.abs(a["U"]).max() - 11.3) < 0.06
    assert b["n_sat"].sum() == 55 and (b["n_sat"] > 0).sum() == 15
    assert c["n_sat"].sum() == 1987 and (c["n_sat"] > 0).all() and c["n_sat"].min() == 40 and c["n_sat"].max() == 87
    falls = c["first_fall"][c["first_fall"] >= 0]
    assert len(falls) == 10 and falls.min() == 36 and falls.max() == 48 and abs(c["X"][..., 2].min() - 0.117) < 1e-3
    assert d["n_sat"].sum() == 125 and (d["n_sat"] > 0).sum() == 19 and (d["first_fall"] == -1).all()


def test_oracle_walk_long_window_gives_the_recorded_figures(oracle_lib):
    """Case E: trot 4 x 50, B = 2, R = 4, 2 AL x 4 DDP, the whole 200-step window with the switches of D."""
    phases = pkg.problems.wb_trot_problem()
    so = pkg.Solver(oracle_lib, phases, batch=2)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(pkg.problems.wb_ensemble_x0(2, 20241222)); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 4, 0.02, 0.2, seed=20241222)
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    w = mc.oracle_walk(pkg, oracle_lib, phases, mc.policy_of(so), sc.step_map(phases, 200), xs, d, k)
    print(f"[mc] case E: n_sat {int(w['n_sat'].sum())} on {int((w['n_sat'] > 0).sum())} samples, torque margin {w['sat_margin'].min():.2e}, lowest {w['X'][..., 2].min():.3f}")
    assert np.isfinite(w["X"]).all() and (w["first_bad"] == -1).all()
    assert w["n_sat"].sum() == 6 and (w["n_sat"] > 0).sum() == 3 and (w["first_fall"] == -1).all()
    so.close()


@pytest.fixture(scope="module")
def mc_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mc_emu") / "libhsddp_mc_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "mc_emu.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.mc_emu_draw.restype = ctypes.c_double
    lib.mc_emu_draw.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong]
    assert lib.mc_emu_park_doubles() == 26
    return lib


def emu_disturbed(lib, so, b, x0, smap, d, kick, keep_traj=True):
    """The host build of the disturbed program on problem b of a solved oracle handle; x0, kick: [R, 36]."""
    nph = len(so.phases)
    D = [p["desc"] for p in so.phases]
    hor = np.array([q.horizon for q in D], dtype=np.int32); dt = np.array([q.dt for q in D]); al = np.array([q.BG_alpha for q in D])
    ct = np.array([[q.contact[l] for l in range(4)] for q in D], dtype=np.int32)
    td = np.array([[1 if (q.contact[l] == 0 and q.next_contact[l] == 1) else 0 for l in range(4)] for q in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]      # column-major 12 x 36 per knot
    ptrs = lambda arrs: (ctypes.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n, R = smap.shape[1], x0.shape[0]
    x0 = np.ascontiguousarray(x0)
    xf = np.zeros((R, 36)); rows = np.zeros((R, 5)); X = np.zeros((R, n + 1, 36)); U = np.zeros((R, n, 12)); extra = np.zeros((R, 2))
    sw = np.array([d.sigma_u, d.sigma_q, d.sigma_v, d.u_max, d.fall_height])
    kick = None if kick is None else np.ascontiguousarray(kick)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.mc_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), ctypes.c_double(mc.PSI_DYN), vp(smap), n, R, vp(x0), vp(xf), vp(rows),
                        vp(X) if keep_traj else None, vp(U) if keep_traj else None, ctypes.c_ulonglong(d.seed), d.first_problem + b, vp(sw), d.kick_step,
                        None if kick is None else vp(kick), vp(extra))
    assert rc == 0
    return xf, rows, X, U, extra


def to_result(xf, rows, X, U, extra):
    r = np.zeros(rows.shape[:-1], dtype=pkg._abi.SIM_ROW_DTYPE)
    for i, f in enumerate(("dev_q", "dev_v", "min_height", "max_torque", "first_bad")):
        r[f] = rows[..., i]
    e = np.zeros(extra.shape[:-1], dtype=pkg._abi.MC_EXTRA_DTYPE)
    e["first_fall"] = extra[..., 0]; e["n_sat"] = extra[..., 1]
    return dict(rows=r, x_final=xf, X=X, U=U, extra=e)


def test_host_uniforms_are_bit_equal_to_numpy(mc_emu):
    for seed in (0, 11, 20241222, (1 << 64) - 1):
        rng = pkg.problems.SplitMix64(seed)
        assert [mc_emu.mc_emu_draw(seed, n) for n in range(1, 200)] == [rng.next() for _ in range(199)]
        n0 = 2 * ((((7 * 65536) + 5) * 65536 + 199) * 48 + 47)
        rng = pkg.problems.SplitMix64(seed); rng.skip(n0)
        assert mc_emu.mc_emu_draw(seed, n0 + 1) == rng.next() and mc_emu.mc_emu_draw(seed, n0 + 2) == rng.next()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_disturbed_program_on_the_host_matches_the_oracle_walk(mc_emu, solved_trot, walks, name):
    """Trajectories, rows and extras of the 48-step window (a lift-off and both touchdowns) under cases A - D."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    d, k = mc.cases(pkg, xs.shape[:2])[name]
    outs = [emu_disturbed(mc_emu, so, b, xs[b], smap, d, None if k is None else k[b]) for b in range(4)]
    res = to_result(*[np.stack([o[i] for o in outs]) for i in range(5)])
    mc.compare_disturbed(f"host {name}", res, walks[name], mc.xbar_window(pol, smap))
    lean = emu_disturbed(mc_emu, so, 1, xs[1], smap, d, None if k is None else k[1], keep_traj=False)      # without trajectories: same rows, extras, final states
    assert np.array_equal(lean[0], outs[1][0]) and np.array_equal(lean[1], outs[1][1]) and np.array_equal(lean[4], outs[1][4])


def test_disturbed_program_on_the_host_shards_and_extends(mc_emu, oracle_lib, solved_trot):
    """first_problem = 5 draws the numbers of problems 5 + b (case A against the walk); a 24-step window is the head of the 48-step one (case D)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    d, _ = mc.cases(pkg, xs.shape[:2])["A"]
    d.first_problem = 5
    ref = mc.oracle_walk(pkg, oracle_lib, phases, pol, smap, xs, d)
    print(f"[mc] case A, first_problem 5: dev_q {np.abs(ref['X'][..., :18] - mc.xbar_window(pol, smap)[:, None, :, :18]).max():.3f}, max |u| {np.abs(ref['U']).max():.2f}")
    outs = [emu_disturbed(mc_emu, so, b, xs[b], smap, d, None) for b in range(4)]
    res = to_result(*[np.stack([o[i] for o in outs]) for i in range(5)])
    mc.compare_disturbed("host A first_problem 5", res, ref, mc.xbar_window(pol, smap))
    d, k = mc.cases(pkg, xs.shape[:2])["D"]
    long = emu_disturbed(mc_emu, so, 2, xs[2], smap, d, k[2])
    short = emu_disturbed(mc_emu, so, 2, xs[2], sc.step_map(phases, 24), d, k[2])
    assert np.array_equal(short[2][:, :24], long[2][:, :24]) and np.array_equal(short[3], long[3][:, :24])
    one = emu_disturbed(mc_emu, so, 2, xs[2][:1], smap, d, k[2][:1])      # sample 0 alone: the same numbers
    assert np.array_equal(one[2][0], long[2][0]) and np.array_equal(one[4][0], long[4][0])


def test_multiphase_ddp_header_compiles_with_disturbed_runs(tmp_path):
    """The C++ mirror: Simulation::run(x0, dist, kick) and the extras of SimResult compile, inline, without the library."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0, const double* kick) {\n'
                   '    hsddp_mc_dist_t d = hsddp::default_disturbance(); d.sigma_u = 0.2; d.u_max = 17.0; d.kick_step = 3;\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8); sim.run(x0, d, kick); hsddp::SimResult r = sim.result();\n'
                   '    (void)r.extra[0].first_fall; (void)r.extra[0].n_sat; sim.run(x0, d, nullptr, 1, 0); sim.run(x0);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
