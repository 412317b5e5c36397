"""CPU tests of the policy latency of the MPC episodes (include/hsddp_latency.h): the numpy definition compose_policy against the host build of the
kernel body (tests/_emu/latency_emu.cpp, epi_latency of cafe-mpc_amd/csrc/episode.hpp) bit for bit, the host rule of
cafe-mpc_amd/csrc/latency_plan.hpp in a stand-alone program under the sanitizers, and the ABI mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import episode_common as ec

A = pkg._abi
ep = pkg.episode


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib = ec.build_host(tmp_path_factory.mktemp("latency_emu"), "latency_emu.cpp", "libhsddp_latency_emu.so")
    assert lib.latency_emu_row_doubles() == A.LATENCY_ROW == 516
    return lib


def random_policy(rng, B, horizons):
    """{phase: (XBAR [B, h+1, 36], UBAR [B, h, 12], K [B, h, 12, 36])} as Solver.field returns them."""
    return {p: (rng.standard_normal((B, h + 1, 36)), rng.standard_normal((B, h, 12)), rng.standard_normal((B, h, 12, 36))) for p, h in enumerate(horizons)}


def emu_tick(lib, fields, horizons, B, n, D, valid, lmap, delay, n_stale, end_reason, prev):
    """One launch of the host build on the handle arrays of `fields`: (effective rows in the device's layout Xe, Ue, Ke, the next stash)."""
    nph = len(horizons)
    xb = [np.ascontiguousarray(fields[p][0]) for p in range(nph)]; ub = [np.ascontiguousarray(fields[p][1]) for p in range(nph)]
    kk = [np.ascontiguousarray(fields[p][2].transpose(0, 1, 3, 2)) for p in range(nph)]      # column-major 12 x 36 per knot, the handle's order
    ptrs = lambda arrs: (ctypes.c_void_p * nph)(*[a.ctypes.data for a in arrs])
    Xe = np.full((n, B, 72), np.nan); Ue = np.full((n, B, 12), np.nan); Ke = np.full((n, B, 432), np.nan)
    nxt = np.full((B, max(D, 1), 516), np.nan)
    rc = lib.latency_emu_run(nph, ec.vp(np.ascontiguousarray(horizons, dtype=np.int32)), ptrs(xb), ptrs(ub), ptrs(kk), B, n, D, 1 if valid else 0,
                             ec.vp(np.ascontiguousarray(lmap, dtype=np.int32)), ec.vp(delay), ec.vp(n_stale), ec.vp(end_reason), ec.vp(prev), ec.vp(nxt), ec.vp(Xe), ec.vp(Ue), ec.vp(Ke))
    assert rc == 0
    return Xe, Ue, Ke, nxt[:, :D]


def problem_major(lib, B, n, b0, nb, Xe, Ue, Ke):
    Xo = np.zeros((nb, n, 72)); Uo = np.zeros((nb, n, 12)); Ko = np.zeros((nb, n, 432))
    assert lib.latency_emu_get_policy(B, n, b0, nb, ec.vp(Xe), ec.vp(Ue), ec.vp(Ke), ec.vp(Xo), ec.vp(Uo), ec.vp(Ko)) == 0
    return np.concatenate([Xo, Uo, Ko], axis=2)


def long_map(horizons, L):
    out = [[p, k, 0] for p, h in enumerate(horizons) for k in range(h)][:L]
    return np.ascontiguousarray(np.array(out, dtype=np.int32).T)


def test_compose_policy_is_the_host_build_of_the_kernel_bit_for_bit(emu):
    """B = 5, n_exec = 3, delays [0, 1, 2, 3, 0] (D = n_exec), two phases of 2 and 4 knots so that the tick and the stash both cross the boundary:
    a first tick without a valid stash, a second one on another policy with it; robot 2 frozen; a slice with a b0 offset."""
    B, n = 5, 3
    horizons = (2, 4)
    delay = np.array([0, 1, 2, 3, 0], dtype=np.int32); D = int(delay.max())
    lmap = long_map(horizons, n + D)
    rng = np.random.default_rng(20250101)
    n_stale = np.zeros(B, dtype=np.int32); frozen = np.array([0, 0, 2, 0, 0], dtype=np.int32)
    f0 = random_policy(rng, B, horizons)
    rows0 = ep.policy_rows(None, lmap, fields=f0)      # [B, n + D, 516]
    assert rows0.shape == (B, n + D, 516)
    Xe, Ue, Ke, stash = emu_tick(emu, f0, horizons, B, n, D, False, lmap, delay, n_stale, frozen, np.full((B, D, 516), np.nan))
    want0 = ep.compose_policy(None, rows0[:, :n], delay, False)
    assert problem_major(emu, B, n, 0, B, Xe, Ue, Ke).tobytes() == want0.tobytes() and want0.tobytes() == rows0[:, :n].tobytes()
    assert stash.tobytes() == np.ascontiguousarray(rows0[:, n:]).tobytes()
    assert not n_stale.any()      # nothing was stale: no stash
    # the terminal knot is the second half of the X part on a phase's last knot: step 1 is knot 1 of phase 0 (h = 2)
    assert np.array_equal(want0[:, 1, 36:72], f0[0][0][:, 2]) and np.array_equal(want0[:, 2, :36], f0[1][0][:, 0])
    f1 = random_policy(rng, B, horizons)
    rows1 = ep.policy_rows(None, lmap, fields=f1)
    Xe, Ue, Ke, stash1 = emu_tick(emu, f1, horizons, B, n, D, True, lmap, delay, n_stale, frozen, np.ascontiguousarray(stash))
    want1 = ep.compose_policy(rows0[:, n:], rows1[:, :n], delay, True)
    got1 = problem_major(emu, B, n, 0, B, Xe, Ue, Ke)
    assert got1.tobytes() == want1.tobytes()
    for b in range(B):      # the definition, spelt out
        for s in range(n):
            assert np.array_equal(want1[b, s], rows0[b, n + s] if s < delay[b] else rows1[b, s])
    assert not np.array_equal(want1[3], rows1[3, :n]) and np.array_equal(want1[0], rows1[0, :n])
    assert stash1.tobytes() == np.ascontiguousarray(rows1[:, n:]).tobytes()
    assert list(n_stale) == [0, 1, 0, 3, 0]      # the frozen robot (delay 2) is composed like the others and counts nothing
    assert np.array_equal(want1[2, :2], rows0[2, n:n + 2])
    assert problem_major(emu, B, n, 1, 3, Xe, Ue, Ke).tobytes() == np.ascontiguousarray(want1[1:4]).tobytes()      # a b0 offset
    Xs, Us, Ks = ep.split_policy(want1)
    assert Xs.shape == (B, n, 2, 36) and Us.shape == (B, n, 12) and Ks.shape == (B, n, 432) and np.array_equal(Ks[4, 1].reshape(36, 12).T, f1[0][2][4, 1])


def test_latency_plan_rule_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/latency_plan_table.cpp, a stand-alone program around the host rule (cafe-mpc_amd/csrc/latency_plan.hpp): stale steps on a phase's last
    knot, on both sides of a boundary with a reset map, D = n_exec, the pending impact, a window one knot too short.  Compiled with
    -fsanitize=address,undefined and run directly; it has to finish clean."""
    exe = str(tmp_path / "latency_plan_table")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "latency_plan_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "latency_plan_table: clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_latency_step_map_is_the_rule_of_the_simulation_object():
    import sim_common
    pd, phases, cfg, _, _, n = ec.bound_problem(pkg)
    for L in (n, n + 1, 2 * n):
        assert np.array_equal(ep.latency_step_map(phases, L), sim_common.step_map(phases, L))
    with pytest.raises(ValueError):
        ep.latency_step_map(phases, 10 ** 6)


def test_latency_abi_mirror_matches_the_header(tmp_path):
    """Every prototype of include/hsddp_latency.h is in LATENCY_EXPORTS and in no other list; hsddp_latency_row_t field for field."""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsddp_latency.h")).read(), flags=re.S)
    protos = set(re.findall(r"\b(hsddp_[a-z_]+)\s*\(", code))
    assert protos == set(A.LATENCY_EXPORTS) and len(protos) == 3
    for other in (A.EXPORTS, A.SIM_EXPORTS, A.MC_EXPORTS, A.GRF_EXPORTS, A.EPISODE_EXPORTS):
        assert not protos & set(other)
    names = [n for n, _ in A.LatencyRow._fields_]
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp_latency.h"\nint main(void){ printf("%zu", sizeof(hsddp_latency_row_t));\n'
                    + "".join(f'printf(" %zu", offsetof(hsddp_latency_row_t, {n}));\n' for n in names) + 'printf("\\n"); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [ctypes.sizeof(A.LatencyRow)] + [getattr(A.LatencyRow, n).offset for n in names] == [8, 0, 4]
    assert A.LATENCY_ROW_DTYPE.itemsize == 8 and [A.LATENCY_ROW_DTYPE.fields[n][1] for n in names] == got[1:]


def test_hip_library_exports_the_latency_symbols(oracle_lib):
    if not os.path.exists(pkg.HIP_LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc")])
    lib = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for s in A.LATENCY_EXPORTS:
        assert hasattr(lib, s), s
    A.bind_latency(lib)
    assert len(lib.hsddp_latency_set.argtypes) == 4 and len(lib.hsddp_latency_get_policy.argtypes) == 6
    with pytest.raises(RuntimeError):       # the CPU checker keeps the shared ABI only
        A.bind_latency(oracle_lib)


def test_multiphase_ddp_header_compiles_with_latency(tmp_path):
    """The C++ mirror: hsddp::Episode::set_latency / latency compile, and so does the harness tests/cpp/latency_loop.cpp (linked and run in
    tests/test_latency_gpu.py)."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::Episode& e, const int* d) { e.set_latency(true, d); e.set_latency(true, nullptr, 1); e.set_latency(false); (void)e.latency()[0].n_stale; }\n')
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host")]
    subprocess.check_call(["g++", "-std=c++17", "-c"] + inc + [str(src), "-o", str(tmp_path / "w.o")])
    subprocess.check_call(["g++", "-std=c++17", "-c"] + inc + [os.path.join(ROOT, "tests", "cpp", "latency_loop.cpp"), "-o", str(tmp_path / "l.o")])
