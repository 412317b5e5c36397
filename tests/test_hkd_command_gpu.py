"""HKD-MPC command export on the MI355X (include/hsddp_hkd.h, csrc/hkd_pack.hpp k_pack_hkd): rows bit-equal to the numpy specification
hkd_command.pack_rows on the same handle's fields (fp64 and fp32 handles, host and device destinations, sub-ranges, the single-problem call),
parity with the CPU checker, the receding-horizon loop with an export every tick, argument checks, and the C++ harness tests/cpp/hkd_mpc_loop.cpp."""
import ctypes
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT

TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")
builder = importlib.import_module(pkg.__name__ + ".builder")
hkd_command = importlib.import_module(pkg.__name__ + ".hkd_command")
EPS32 = float(np.finfo(np.float32).eps)


def bound_problem_data():
    cp = builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info"))
    return builder.HKDProblemData(builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True), cp)


def ddp_setting(al, ddp):
    opt = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info"))
    opt.max_AL_iter, opt.max_DDP_iter = al, ddp
    return opt


def fixture_x0(info, batch, seed=3):
    rng = np.random.default_rng(seed)
    x0 = np.tile(info["x0"], (batch, 1))
    x0[:, :12] += rng.uniform(-0.01, 0.01, (batch, 12))
    return x0


def solved(lib, phases, x0, opt, **kw):
    s = pkg.Solver(lib, phases, batch=x0.shape[0], **kw)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    s.solve(opt)
    return s


@pytest.fixture(scope="module")
def fixture_f64(hip_lib):
    phases, info = bound_problem_data().describe()
    s = solved(hip_lib, phases, fixture_x0(info, 64), ddp_setting(1, 2))
    yield s, info
    s.close()


def check_bit_equal(s, info_st, batch, n_steps, seed):
    rng = np.random.default_rng(seed)
    pf = rng.standard_normal((batch, 12)).astype(np.float32)
    kw = dict(n_steps=n_steps, mpc_time=0.12 + n_steps, dt=0.01, status_times=info_st)
    rows = s.export_hkd_commands(0, batch, pf=pf, **kw)
    spec = hkd_command.pack_rows(s, 0, batch, pf=pf, **kw)
    assert rows.shape == (batch, 1954)
    bad = np.nonzero((rows != spec).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], np.nonzero(rows[bad[0]] != spec[bad[0]])[0][:16])
    return rows, pf, kw


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [1, 9, 10])
def test_batched_rows_bit_equal_to_the_specification_f64(fixture_f64, n_steps):
    s, info = fixture_f64
    rows, pf, kw = check_bit_equal(s, info["status_durations"], 64, n_steps, 11 + n_steps)
    for b in (0, 17, 63):      # the single-problem call is its row of the batched call
        assert np.array_equal(s.export_hkd_command(b, pf=pf[b], **kw)["raw"], rows[b])
    sub = s.export_hkd_commands(5, 20, pf=pf[5:25], **kw)      # b0 > 0, nb < batch
    assert np.array_equal(sub, rows[5:25])
    rt = ctypes.CDLL("libamdhip64.so.7")                        # the HIP runtime libhsddp_hip.so itself runs on (device destination)
    p = ctypes.c_void_p()
    assert rt.hipMalloc(ctypes.byref(p), ctypes.c_size_t(rows.nbytes + 8)) == 0
    try:
        for off, b0, nb in ((0, 0, 64), (4, 5, 20)):          # an 8-byte aligned destination and one that is only 4-byte aligned
            assert rt.hipMemset(p, ctypes.c_int(0xff), ctypes.c_size_t(rows.nbytes + 8)) == 0
            assert s.export_hkd_commands(b0, nb, pf=pf[b0:b0 + nb], out=p.value + off, **kw) == p.value + off
            dev = np.zeros((nb, 1954), dtype=np.uint32)
            assert rt.hipMemcpy(ctypes.c_void_p(dev.ctypes.data), ctypes.c_void_p(p.value + off), ctypes.c_size_t(dev.nbytes), 2) == 0      # hipMemcpyDeviceToHost
            assert np.array_equal(dev, rows[b0:b0 + nb]), off
    finally:
        rt.hipFree(p)
    nopf = s.export_hkd_commands(0, 64, n_steps=n_steps, mpc_time=kw["mpc_time"], dt=0.01)      # no status times, no pf_in: zeros there
    assert np.array_equal(nopf, hkd_command.pack_rows(s, 0, 64, n_steps=n_steps, mpc_time=kw["mpc_time"], dt=0.01))


@pytest.mark.gpu
def test_batched_rows_bit_equal_f32_config5(hip_lib):
    """An fp32 handle at config-5 phases (problems.hkd_bound_problem, N = 200), batch 256."""
    phases = pkg.problems.hkd_bound_problem()
    x0 = pkg.problems.hkd_ensemble_x0(256, 20241220, phases)
    s = solved(hip_lib, phases, x0, pkg.problems.hkd_ddp_setting(max_AL_iter=1, max_DDP_iter=2), precision=pkg.PREC_F32)
    st = np.arange(len(phases) * 4, dtype=np.float64).reshape(-1, 4) * 0.05 + 0.1
    rows, pf, kw = check_bit_equal(s, st, 256, 9, 5)
    assert np.array_equal(s.export_hkd_commands(100, 156, pf=pf[100:], **kw), rows[100:])
    s.close()


@pytest.mark.gpu
def test_rows_match_the_oracle(hip_lib, oracle_lib):
    """The GPU rows, decoded, against pack_rows on the CPU checker after the same solve.  Tolerances: the HKD parity tolerances (fields rtol 1e-6
    of their scale, gains 1e-6 absolute) plus the fp32 rounding of both sides."""
    phases, info = bound_problem_data().describe()
    x0 = fixture_x0(info, 4, seed=9)
    opt = ddp_setting(2, 2)
    sg, so = solved(hip_lib, phases, x0, opt), solved(oracle_lib, phases, x0, opt)
    pf = np.random.default_rng(1).standard_normal((4, 12)).astype(np.float32)
    kw = dict(n_steps=9, mpc_time=0.5, dt=0.01, status_times=info["status_durations"], pf=pf)
    g = hkd_command.decode(sg.export_hkd_commands(0, 4, **kw))
    o = hkd_command.decode(hkd_command.pack_rows(so, 0, 4, **kw))
    for name in ("N_mpcsteps", "mpc_times", "contacts", "statusTimes"):
        assert np.array_equal(g[name], o[name]), name
    for name, tol in (("feedback", 1e-6), ("hkd_controls", None), ("des_body_state", None), ("foot_placement", None)):
        a, b = o[name].astype(np.float64), g[name].astype(np.float64)
        sc = max(1.0, np.abs(a).max())
        t = (tol if tol is not None else 1e-6 * sc) + 2 * EPS32 * np.abs(a).max()
        assert np.abs(a - b).max() <= t, (name, np.abs(a - b).max(), t)
    sg.close(); so.close()


@pytest.mark.gpu
def test_receding_horizon_loop_with_export(hip_lib):
    """The 10-tick loop of test_hkd_receding_horizon_loop_parity on the GPU with an export every tick: rows equal the specification, footholds
    equal builder.hkd_next_footholds (pf_in for the legs it does not find), the durations are the builder's, and a warm tick allocates nothing."""
    pd = bound_problem_data()
    phases, info = pd.describe()
    x0 = np.vstack([info["x0"], info["x0"]]); x0[1, :12] += 0.01
    s = solved(hip_lib, phases, x0, ddp_setting(2, 4))
    opt_rt = ddp_setting(2, 1)
    pf = np.tile(pd.ref.at(np.float32(0))["foot_placements"].astype(np.float32), (2, 1))
    mallocs, ph = [], phases
    for tick in range(1, 11):
        m = pd.update()
        ph, inf = builder.shift_solver_in_place(s, ph, pd, m)
        s.set_control_knot(0, 0, None)
        s.set_initial_condition(np.ascontiguousarray(s.field(0, "XBAR")[:, 0])); s.solve(opt_rt)
        kw = dict(n_steps=9, mpc_time=0.02 * tick, dt=0.01, status_times=inf["status_durations"], pf=pf)
        rows = s.export_hkd_commands(0, 2, **kw)
        assert np.array_equal(rows, hkd_command.pack_rows(s, 0, 2, **kw)), tick
        d = hkd_command.decode(rows)
        for b in range(2):
            found = builder.hkd_next_footholds(s, inf["contacts"], problem=b)
            for l in range(4):
                assert np.array_equal(d["foot_placement"][b, 3 * l:3 * l + 3], found[l] if l in found else pf[b, 3 * l:3 * l + 3]), (tick, b, l)
        pf = d["foot_placement"].copy()
        mallocs.append(hip_lib.hsddp_debug_malloc_count())
    assert mallocs[3:] == [mallocs[3]] * len(mallocs[3:]), mallocs      # flat from tick 4 on
    s.close()


@pytest.mark.gpu
def test_export_argument_checks(hip_lib, fixture_f64):
    pkg._abi.bind_hkd(hip_lib)
    s, info = fixture_f64
    out = np.zeros((64, 1954), dtype=np.uint32)
    call = lambda h, b0, nb, n: hip_lib.hsddp_export_hkd_commands(h, b0, nb, n, 0.0, 0.01, None, None, out.ctypes.data, 0)
    EINVAL = -1
    assert call(s.h, 0, 64, 9) == 0
    for n in (0, 11):
        assert call(s.h, 0, 1, n) == EINVAL
    for b0, nb in ((-1, 1), (0, 65), (60, 5), (64, 1), (0, -1)):
        assert call(s.h, b0, nb, 9) == EINVAL, (b0, nb)
    assert hip_lib.hsddp_export_hkd_command(s.h, 64, 9, 0.0, 0.01, None, None, out.ctypes.data) == EINVAL
    short = pkg.problems.hkd_bound_problem(n_knots=8)      # 6 + 2 control knots
    ss = solved(hip_lib, short, pkg.problems.hkd_ensemble_x0(2, 1, short), ddp_setting(1, 1))
    assert call(ss.h, 0, 2, 8) == 0 and call(ss.h, 0, 2, 9) == EINVAL
    ss.close()
    wb = pkg.problems.wb_trot_problem(schedule=((0, 1, 1, 0), (1, 0, 0, 1)), horizons=(8, 8), last_next=(0, 1, 1, 0))
    sw = pkg.Solver(hip_lib, wb, batch=2)
    assert call(sw.h, 0, 2, 9) == EINVAL
    sw.close()


def python_hkd_loop(lib, n_ticks, opt0):
    """tests/cpp/hkd_mpc_loop.cpp through ctypes: same builder, same solves, the previous message's footholds as the next pf_in."""
    pd = bound_problem_data()
    phases, info = pd.describe()
    s = solved(lib, phases, info["x0"][None, :], opt0)
    opt_rt = ddp_setting(2, 1)
    pf = pd.ref.at(np.float32(0))["foot_placements"].astype(np.float32)
    pf = s.export_hkd_command(0, 9, 0.0, 0.01, info["status_durations"], pf)["foot_placement"]
    rows, ph = [], phases
    for tick in range(1, n_ticks + 1):
        m = pd.update()
        ph, inf = builder.shift_solver_in_place(s, ph, pd, m)
        s.set_control_knot(0, 0, None)
        s.set_initial_condition(np.ascontiguousarray(s.field(0, "XBAR")[:, 0])); s.solve(opt_rt)
        d = s.export_hkd_command(0, 9, 0.02 * tick, 0.01, inf["status_durations"], pf)
        rows.append(d["raw"]); pf = d["foot_placement"]
    s.close()
    return rows


@pytest.mark.gpu
def test_cpp_hkd_mpc_loop_on_the_hip_library(hip_lib, tmp_path):
    """tests/cpp/hkd_mpc_loop.cpp (C++ HkdProblemData + hsddp::MultiPhaseDDP<double>::export_hkd_command) linked against libhsddp_hip.so: its
    rows equal the ctypes path's tick by tick (solve_time aside: a wall-clock figure), no device allocation once warm."""
    exe = tmp_path / "hkd_mpc_loop"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "hkd_mpc_loop.cpp"), "-L", os.path.join(ROOT, "cafe-mpc_amd"), "-lhsddp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cafe-mpc_amd"), "-o", str(exe)])
    opt0 = ddp_setting(2, 4)
    (tmp_path / "opt.bin").write_bytes(bytes(opt0))
    out = json.loads(subprocess.check_output([str(exe), TREE, "bound", str(tmp_path / "opt.bin"), "10"], timeout=600))
    print("C++ HKD MPC loop:", {k: v for k, v in out.items() if k.endswith("_mean")})
    rows = python_hkd_loop(hip_lib, 10, opt0)
    solve_w = hkd_command.OFFSETS["solve_time"]
    for tick, (a, b) in enumerate(zip(out["rows"], rows), 1):
        a = np.array(a, dtype=np.uint32)
        assert np.array_equal(np.delete(a, solve_w), np.delete(b, solve_w)), (tick, np.nonzero(np.delete(a, solve_w) != np.delete(b, solve_w))[0][:16])
        assert np.array_equal(np.array(out["foot_placement"][tick - 1], dtype=np.float32), hkd_command.decode(a)["foot_placement"])
    assert out["device_allocations_in_warm_ticks"] == 0
    assert 0 < out["export_ms_mean"] < out["total_ms_mean"]
