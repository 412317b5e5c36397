"""CPU tests of the closed-loop policy simulation (include/hsddp_sim.h): the ctypes mirror, the perturbed initial states, and the simulation
program itself (cafe-mpc_amd/csrc/wb_sim.hpp) compiled for the host by tests/_emu/sim_emu.cpp - the four lanes of a quad evaluated together -
against reference values from the oracle's existing entry points (tests/sim_common.py).  Real HIP execution: tests/test_sim_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc


def test_sim_abi_mirror_matches_the_header(tmp_path):
    """hsddp_sim_row_t field for field, and every prototype of include/hsddp_sim.h has a bound mirror."""
    src = open(os.path.join(ROOT, "include", "hsddp_sim.h")).read()
    body = re.search(r"typedef struct hsddp_sim_row \{(.*?)\} hsddp_sim_row_t;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), ty) for n in names.split(",")]
    Row = pkg._abi.SimRow
    assert [(n, {"double": ctypes.c_double, "int": ctypes.c_int}[t]) for n, t in fields] == list(Row._fields_)
    assert ctypes.sizeof(Row) == 40 and Row.dev_q.offset == 0 and Row.max_torque.offset == 24 and Row.first_bad.offset == 32
    assert pkg._abi.SIM_ROW_DTYPE.itemsize == 40 and pkg._abi.SIM_ROW_DTYPE.names == tuple(n for n, _ in Row._fields_)
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp_sim.h"\nint main(void){ printf("%zu %zu %zu\\n", sizeof(hsddp_sim_row_t), '
                    'offsetof(hsddp_sim_row_t, max_torque), offsetof(hsddp_sim_row_t, first_bad)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == [ctypes.sizeof(Row), Row.max_torque.offset, Row.first_bad.offset]
    protos = set(re.findall(r"\b(hsddp_sim_[a-z_]+)\s*\(", src))
    assert protos == set(pkg._abi.SIM_EXPORTS) and len(protos) == 7

    class Fake:      # bind_sim attaches prototypes to whatever has the symbols, and refuses a library that lacks one
        pass
    lib = Fake()
    for s in pkg._abi.SIM_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        pkg._abi.bind_sim(lib)
    setattr(lib, pkg._abi.SIM_EXPORTS[-1], Fake())
    pkg._abi.bind_sim(lib)
    assert lib.hsddp_sim_device_final.restype is ctypes.c_void_p and len(lib.hsddp_sim_create.argtypes) == 5


def test_perturbed_states_are_seeded_and_keep_sample_zero():
    x = pkg.problems.wb_ensemble_x0(3, 7)
    a = pkg.problems.perturbed_states(x, 5, 0.02, 0.2, seed=11)
    assert a.shape == (3, 5, 36) and a.dtype == np.float64
    assert np.array_equal(a[:, 0], x)
    assert np.array_equal(a, pkg.problems.perturbed_states(x, 5, 0.02, 0.2, seed=11))
    assert not np.array_equal(a, pkg.problems.perturbed_states(x, 5, 0.02, 0.2, seed=12))
    assert np.array_equal(a[1:], pkg.problems.perturbed_states(x[1:], 5, 0.02, 0.2, seed=11, first=1))      # a shard reproduces its slice
    d = pkg.problems.perturbed_states(np.zeros((1, 36)), 2001, 0.02, 0.2, seed=3)[0, 1:]
    assert abs(d[:, :18].std() / 0.02 - 1) < 0.05 and abs(d[:, 18:].std() / 0.2 - 1) < 0.05 and abs(d[:, :18].mean()) < 2e-3
    assert np.array_equal(pkg.problems.perturbed_states(x, 4, np.zeros(18), 0.0, seed=1), np.repeat(x[:, None], 4, axis=1))
    with pytest.raises(ValueError):
        pkg.problems.perturbed_states(x, 0, 0.02, 0.2, seed=1)


@pytest.fixture(scope="module")
def sim_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sim_emu") / "libhsddp_sim_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_emu", "sim_emu.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    assert lib.sim_emu_row_doubles() == 5
    return lib


def emu_simulate(lib, so, b, x0, smap, keep_traj=True):
    """The host build of the simulation program on problem b of a solved oracle handle; x0: [R, 36]."""
    nph = len(so.phases)
    D = [p["desc"] for p in so.phases]
    hor = np.array([d.horizon for d in D], dtype=np.int32); dt = np.array([d.dt for d in D]); al = np.array([d.BG_alpha for d in D])
    ct = np.array([[d.contact[l] for l in range(4)] for d in D], dtype=np.int32)
    td = np.array([[1 if (d.contact[l] == 0 and d.next_contact[l] == 1) else 0 for l in range(4)] for d in D], dtype=np.int32)
    xb = [np.ascontiguousarray(so.field(i, "XBAR", b, 1)[0]) for i in range(nph)]
    ub = [np.ascontiguousarray(so.field(i, "UBAR", b, 1)[0]) for i in range(nph)]
    kk = [np.ascontiguousarray(so.field(i, "K", b, 1)[0].transpose(0, 2, 1)) for i in range(nph)]      # back to column-major 12 x 36 per knot
    ptrs = lambda arrs: (ctypes.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    n, R = smap.shape[1], x0.shape[0]
    x0 = np.ascontiguousarray(x0)
    xf = np.zeros((R, 36)); rows = np.zeros((R, 5)); X = np.zeros((R, n + 1, 36)); U = np.zeros((R, n, 12))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.sim_emu_run(nph, vp(hor), vp(dt), vp(al), vp(ct), vp(td), ptrs(xb), ptrs(ub), ptrs(kk), ctypes.c_double(3.1415), vp(smap), n, R, vp(x0), vp(xf), vp(rows),
                         vp(X) if keep_traj else None, vp(U) if keep_traj else None)
    assert rc == 0
    return xf, rows, X, U


def to_result(xf, rows, X=None, U=None):
    r = np.zeros(rows.shape[:-1], dtype=pkg._abi.SIM_ROW_DTYPE)
    for i, f in enumerate(("dev_q", "dev_v", "min_height", "max_torque", "first_bad")):
        r[f] = rows[..., i]
    out = dict(rows=r, x_final=xf)
    if X is not None:
        out.update(X=X, U=U)
    return out


@pytest.fixture(scope="module")
def solved_trot(oracle_lib):
    """Row 1 of the issue's table: trot 4 x 12, four problems, 3 AL x 4 DDP iterations, eight samples around Xbar[0] (sigma 0.02 / 0.2)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    x0 = pkg.problems.wb_ensemble_x0(4, 20241222)
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(x0); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    return phases, so, xs


def test_sim_program_on_the_host_matches_the_oracle(sim_emu, solved_trot):
    """Full 48-step window: a lift-off boundary and two touchdown boundaries, so the impact mode of the contact solve is covered here."""
    phases, so, xs = solved_trot
    smap = sc.step_map(phases, 48)
    assert smap[2].sum() == 2 and smap[2][23] == 1 and smap[2][35] == 1 and smap[2][11] == 0
    X, U, xbar = sc.oracle_reference(so, pkg.mhpc_ddp_setting(MS=0), xs, smap)
    assert np.abs(X[:, 1:] - xbar[:, None]).max() > 1e-3          # the samples do leave the plan
    outs = [emu_simulate(sim_emu, so, b, xs[b], smap) for b in range(4)]
    res = to_result(*[np.stack([o[i] for o in outs]) for i in range(4)])
    sc.compare_window("host 48", res, X, U, xbar)
    # without trajectories: same rows and final states; a shorter window ends before the reset map of its last knot
    xf, rows, _, _ = emu_simulate(sim_emu, so, 1, xs[1], smap, keep_traj=False)
    assert np.array_equal(xf, outs[1][0]) and np.array_equal(rows, outs[1][1])
    xf24, _, X24, _ = emu_simulate(sim_emu, so, 1, xs[1], sc.step_map(phases, 24))
    assert np.array_equal(X24[:, :24], outs[1][2][:, :24]) and np.array_equal(xf24, X24[:, -1])
    assert np.array_equal(X24[:, 24, :18], outs[1][2][:, 24, :18])                                      # the reset map keeps the positions
    assert np.abs(outs[1][2][:, 24, 18:] - X24[:, 24, 18:]).max() > 1e-6      # entry 24 of the long window is the state AFTER the impact


def test_sim_program_contains_a_diverging_sample(sim_emu, solved_trot):
    """A sample whose state fails the rollout's divergence test keeps the state it had, reports the step, and leaves the others alone."""
    phases, so, xs = solved_trot
    smap = sc.step_map(phases, 13)
    x = xs[2].copy(); x[3, 18] = 1e7
    xf, rows, X, U = emu_simulate(sim_emu, so, 2, x, smap)
    xf0, rows0, X0, U0 = emu_simulate(sim_emu, so, 2, xs[2], smap)
    assert rows[3, 4] == 0 and np.array_equal(xf[3], x[3]) and np.array_equal(X[3], np.repeat(x[3][None], 14, axis=0))
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert np.array_equal(xf[keep], xf0[keep]) and np.array_equal(rows[keep], rows0[keep]) and np.array_equal(X[keep], X0[keep]) and np.array_equal(U[keep], U0[keep])
    assert (rows0[:, 4] == -1).all()


def test_dispatch_rule_names_every_walk_and_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/sim_pick_table.cpp, a stand-alone program around the rule that picks the walk of a run (cafe-mpc_amd/csrc/sim_pick.hpp): every setting of
    the switches against a name composed from the suffix rules, exactly the 27 product walks reachable, the inert combinations inert.  Compiled with
    -fsanitize=address,undefined and run directly; it has to finish clean."""
    exe = str(tmp_path / "sim_pick_table")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sim_pick_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "sim_pick_table: clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_multiphase_ddp_header_compiles_with_simulate(tmp_path):
    """The C++ mirror: simulate() and hsddp::Simulation compile; code that does not call them still links against a library without the symbols
    (tests/test_abi.py links the header against the oracle)."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0) {\n'
                   '    hsddp::SimResult r = s.simulate(x0, 4, 8, true); (void)r.rows[0].first_bad;\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8); sim.run(x0); r = sim.result(); (void)sim.device_final(); (void)sim.last_error();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
