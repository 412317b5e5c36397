"""Per-problem constraint limits (include/hsddp_limits.h) without a GPU: the whole-body programs with limits under the lane emulator
(tests/_emu/lim_emu.cpp; both programs: the one-wave knots and the lane quad), the loops that write the tables, the ABI and the build.

The reference is tests/lim_common.LimitedOracle: B single-problem oracle handles whose descriptors carry problem b's limits.

1. test_inputs_qualify_and_cover: the B = 17 input (it holds B = 1 and B = 5) qualifies against the long-double oracle at 0.05 x the plain
   tolerances, and its limits put every (family, region) cell of the relaxed barrier somewhere - computed from the stacked oracle's X, U, Y with each
   problem's own limits, only where the descriptor's limit leaves the value above delta.
2. test_programs_with_limits_match_the_stacked_oracle: per-iterate parity at parity_common's plain tolerances (rtol 1e-8, K 1e-6 absolute, two
   iterates, no arbiter), B = 1, 5, 17, both programs; and the guard: LX / LU of every problem with a row of its own differ from a run without limits
   by more than 100 x the tolerance (a program that ignores its row passes neither).
3. test_all_nan_rows_are_no_table: bit for bit.  test_reduced_model_phases_do_not_see_the_limits: MHPC window, bit for bit.
4. test_pack_and_friction_loops_match_numpy: k_pack_limits' and k_lim_mu's loops bit for bit, two phases with different descriptor limits.
5. ABI: the header against the ctypes mirror, every refusal rule, pack_limits, the rules and the loops as a stand-alone program under ASan + UBSan.
6. test_make_resources_lim: every _lim kernel at its twin's waves per SIMD and LDS size, none with scratch, the committed record is this build's.
7. Build: the C++ mirror compiles.
8. test_launch_rule_matches_its_transcription_and_is_clean_under_the_sanitizers: which rollout and LQ kernels a launch uses (roll_pick.hpp), every
   switch setting against a transcription of the launch helpers' former branches, as a stand-alone program under ASan + UBSan.

Real HIP execution: tests/test_limits_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import barrier_common as bc
import lim_common as lc
import parity_common as pc
import pattern_common as pt
import pw_common as pw
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "cafe-mpc_amd", "csrc")
QUALIFY = 0.05
PROGRAMS = {"wave": lc.WAVE, "quad": lc.QUAD}
EINVAL, ENOTSUP = -1, -4


@pytest.fixture(scope="module")
def lim_emu(tmp_path_factory):
    return lc.build_emu(tmp_path_factory.mktemp("lim_emu"))


@pytest.fixture(scope="module")
def inputs(oracle_lib):
    """(phases, x0, rows) at B = 17; the forces the friction coefficients come from are computed once."""
    ph = lc.phases(); x0 = lc.x0_of(17)
    return ph, x0, lc.limit_rows(17, ph, lc.forces(oracle_lib, ph, x0))


def test_inputs_qualify_and_cover(oracle_lib, oracle_ld_lib, inputs):
    ph, x0, rows = inputs
    assert np.array_equal(lc.x0_of(5), x0[:5]) and np.isnan(rows[0]).all()
    only_mu = [b for b in range(17) if not np.isnan(rows[b, lc.MU]) and np.isnan(np.delete(rows[b], lc.MU)).all()]
    only_tq = [b for b in range(17) if not np.isnan(rows[b, lc.TORQUE]) and np.isnan(rows[b, 1:]).all()]
    assert only_mu and only_tq, (only_mu, only_tq)      # the NaN fallback per entry
    so, sx = lc.LimitedOracle(oracle_lib, ph, x0, rows), lc.LimitedOracle(oracle_ld_lib, ph, x0, rows)
    so.hybrid_rollout(0.0, pkg.mhpc_ddp_setting())
    n = len(ph)
    cells = lc.coverage(ph, rows, [so.field(i, "X") for i in range(n)], [so.field(i, "U") for i in range(n)], [so.field(i, "Y") for i in range(n)],
                        [so.field(i, "REB_DELTA") for i in range(n)])
    for fam in lc.FAMILIES:
        for reg in bc.REGIONS:
            hit = sorted({c[0] for c in cells.get((fam, reg), [])})
            print(f"[limits] coverage {fam:10s} {reg:8s}: {len(cells.get((fam, reg), []))} values, rows {hit}")
            assert hit, (fam, reg)
            if reg != "above":
                assert 0 not in hit      # (row 0 has no limits of its own: the descriptor's leave everything above)
    report = pc.run_steps(pkg, so, sx, ph, pkg.mhpc_ddp_setting(), n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
    print(f"[limits] qualify: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    so.close(); sx.close()


@pytest.mark.parametrize("program", list(PROGRAMS))
@pytest.mark.parametrize("batch", lc.BATCHES)
def test_programs_with_limits_match_the_stacked_oracle(lim_emu, oracle_lib, inputs, batch, program):
    lib, raw = lim_emu
    ph, x0, rows = inputs[0], inputs[1][:batch], inputs[2][:batch]
    so = lc.LimitedOracle(oracle_lib, ph, x0, rows)
    se = lc.LimEmu(lib, raw, ph, x0, rows, PROGRAMS[program])
    report = pc.run_steps(pkg, so, se, ph, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[limits] B={batch} {program}: error / tolerance {pt.worst_ratio(report)}")
    # the guard: the same two iterates without limits
    sn = lc.LimEmu(lib, raw, ph, x0, None, PROGRAMS[program]); s0 = lc.LimitedOracle(oracle_lib, ph, x0, np.full_like(rows, np.nan))
    pc.run_steps(pkg, s0, sn, ph, pkg.mhpc_ddp_setting(), n_iter=2)
    for b in range(1, batch):
        ratio = 0.0
        for f in ("LX", "LU"):
            for i in range(len(ph)):
                a, c = se.field(i, f), sn.field(i, f)
                ratio = max(ratio, np.abs(a[b] - c[b]).max() / (1e-8 * max(1.0, np.abs(a).max())))
        print(f"[limits] guard B={batch} {program} problem {b}: |with - without| / tolerance {ratio:.3e}")
        assert ratio > 100.0, (b, ratio)
    for s in (so, se, sn, s0):
        s.close()


@pytest.mark.parametrize("program", list(PROGRAMS))
def test_all_nan_rows_are_no_table(lim_emu, inputs, program):
    """Rows of NaN against no table (the programs without switches in the same places, lane-quad terminal knots included), two iterates: every field
    bit for bit - the resolved rows hold the descriptor's values, the scale table ones."""
    lib, raw = lim_emu
    ph, x0 = inputs[0], inputs[1][:5]
    runs = [lc.LimEmu(lib, raw, ph, x0, r, PROGRAMS[program]) for r in (np.full((5, lc.ROW), np.nan), None)]
    opt = pkg.mhpc_ddp_setting()
    for it in range(2):
        for s in runs:
            s.hybrid_rollout(0.0 if it == 0 else 1.0, opt); s.compute_cost(opt)
            if it == 0:
                s.update_nominal_trajectory()
            s.LQ_approximation(opt); assert s.backward_sweep(0.0).all(); s.linear_rollout(1.0, opt)
        for i in range(len(ph)):
            for f in sum(pc.STEP_FIELDS.values(), []):
                assert runs[0].field(i, f).tobytes() == runs[1].field(i, f).tobytes(), (it, i, f)
    for s in runs:
        s.close()


def _mhpc_rows(batch):
    rows = np.full((batch, lc.ROW), np.nan)
    rows[1:, lc.TORQUE] = np.linspace(9.0, 14.0, batch - 1); rows[1:, lc.MU] = np.linspace(0.3, 0.5, batch - 1); rows[2:, lc.HMIN] = 0.12
    return rows


@pytest.mark.parametrize("program", list(PROGRAMS))
def test_reduced_model_phases_do_not_see_the_limits(lim_emu, program):
    """MHPC window: rollout, LQ approximation and backward sweep from the same state - the single-rigid-body phase's fields are those of a run
    without limits bit for bit (its knots read no row - its own h_min is the descriptor's - and the sweep reaches it before any whole-body knot),
    while the whole-body fields differ."""
    lib, raw = lim_emu
    ph = pw.CASES["mhpc"][0](); x0 = pkg.problems.wb_ensemble_x0(5, pw.CASES["mhpc"][1]); opt = pkg.mhpc_ddp_setting()
    runs = [lc.LimEmu(lib, raw, ph, x0, r, PROGRAMS[program]) for r in (_mhpc_rows(5), None)]
    for s in runs:
        s.hybrid_rollout(0.0, opt); s.compute_cost(opt); s.update_nominal_trajectory(); s.LQ_approximation(opt); assert s.backward_sweep(0.0).all()
    srb = [i for i, p in enumerate(ph) if p["desc"].model != lc.MODEL_WB]
    assert srb
    for i in srb:
        for f in pc.STEP_FIELDS["rollout"] + pc.STEP_FIELDS["lq"] + pc.STEP_FIELDS["sweep"]:
            assert np.array_equal(runs[0].field(i, f), runs[1].field(i, f)), (i, f)
    assert not np.array_equal(runs[0].field(0, "LU")[1:], runs[1].field(0, "LU")[1:])
    for s in runs:
        s.close()


def test_pack_and_friction_loops_match_numpy(lim_emu):
    _, raw = lim_emu
    B, nph = 17, 2
    r = np.random.default_rng(5)
    desc = np.array([[17.0, -0.5, -1.5, 1.5, 0.5, -0.5, 2.5, 0.1, 0.6, -8.0, 8.0, 0.0], [12.0, -0.4, -1.4, 1.6, 0.4, -0.6, 2.4, 0.15, 0.4, -5.0, 5.0, 0.0]])

    def draw(nb):
        a = r.uniform(0.25, 4.0, size=(nb, lc.ROW)); a[r.uniform(size=a.shape) < 0.4] = np.nan
        return a

    def want_res(user):
        return np.stack([np.where(np.isnan(user), desc[p][None, :], user) for p in range(nph)])
    p = lambda a: a.ctypes.data_as(lc.DP)
    user = np.full((B, lc.ROW), -7.0); res = np.full((nph, B, lc.ROW), -7.0); want = np.full((B, lc.ROW), np.nan)
    src = draw(5)
    raw.lim_emu_pack(p(user), p(res), p(desc), B, nph, p(src), 3, 5, 0)      # first call: NaN everywhere, then rows 3..7
    want[3:8] = src
    assert user.tobytes() == want.tobytes() and res.tobytes() == want_res(want).tobytes()
    assert np.array_equal(res[0, 0], desc[0]) and np.array_equal(res[1, 0], desc[1])      # an unset row: each phase's own descriptor
    for b0, nb in ((0, 1), (16, 1), (7, 10), (0, 17)):      # later calls overwrite their range only
        src = np.ascontiguousarray(draw(nb + 2)[1:-1])
        raw.lim_emu_pack(p(user), p(res), p(desc), B, nph, p(src), b0, nb, 1)
        want[b0:b0 + nb] = src
        assert user.tobytes() == want.tobytes() and res.tobytes() == want_res(want).tobytes(), (b0, nb)
    desc = desc[::-1].copy()      # the window moved: the same rows against other descriptors
    raw.lim_emu_pack(p(user), p(res), p(desc), B, nph, None, 0, 0, 2)
    assert user.tobytes() == want.tobytes() and res.tobytes() == want_res(want).tobytes()
    # the friction fill: kappa x the static coefficient of each robot's friction row, one multiply, the other entries untouched
    mu_tab = np.array([[0.6, 0.5], [0.25, 0.2], [0.3, 0.3]]); mu_of = np.ascontiguousarray(r.integers(0, 3, size=B), dtype=np.int32); kappa = 0.7
    raw.lim_emu_friction(p(user), p(res), B, nph, p(mu_tab), mu_of.ctypes.data_as(lc.IP), 1, kappa)
    want[:, lc.MU] = kappa * mu_tab[mu_of, 0]
    assert user.tobytes() == want.tobytes() and res.tobytes() == want_res(want).tobytes()
    # Solver.set_limits' packing
    rows = pkg._abi.pack_limits(torque_limit=12.0, joint_lb=[-0.3, -1.2, 1.8], mu=np.array([0.3, 0.4, 0.5]))
    assert rows.shape == (3, 12) and np.all(rows[:, 0] == 12.0) and np.array_equal(rows[1, 1:4], [-0.3, -1.2, 1.8]) and np.array_equal(rows[:, 8], [0.3, 0.4, 0.5])
    assert np.isnan(rows[:, 4:8]).all() and np.isnan(rows[:, 9:]).all()
    assert np.isnan(pkg._abi.pack_limits(nb=4)).all() and pkg._abi.pack_limits(nb=4).shape == (4, 12)
    for bad in (dict(mu=np.ones((2, 2))), dict(joint_lb=np.ones(4)), dict(mu=np.ones(2), h_min=np.ones(3)), dict(friction=0.3)):
        with pytest.raises(ValueError):
            pkg._abi.pack_limits(**bad)


def test_header_matches_the_ctypes_mirror_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "hsddp_limits.h")).read()
    protos = dict(re.findall(r"^int (hsddp_\w+)\((.*?)\);", text, flags=re.M))
    assert sorted(protos) == sorted(pkg._abi.LIMITS_EXPORTS)
    assert int(re.search(r"#define HSDDP_LIMITS_ROW (\d+)", text).group(1)) == pkg._abi.LIMITS_ROW == lc.ROW
    assert sorted(o for o, w in pkg._abi.LIMITS_FIELDS.values()) == [lc.TORQUE, lc.JLB, lc.JUB, lc.HMIN, lc.MU, lc.JSLB, lc.JSUB]
    lib = pkg._abi.bind_limits(C.CDLL(os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")))
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(args.split(",")), name
        for ct, decl in zip(fn.argtypes, args.split(",")):
            assert ct is (C.c_void_p if "*" in decl else C.c_double if "double" in decl else C.c_int), (name, decl)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")], capture_output=True, text=True, check=True).stdout
    for name in pkg._abi.LIMITS_EXPORTS:
        assert re.search(rf" T {name}$", nm, flags=re.M), name
    for k in ("k_rollout_lim", "k_rollout_quad_lim", "k_lq_lim", "k_pack_limits", "k_lim_mu"):      # the library runs its own kernels
        assert k in open(os.path.join(CSRC, "hsddp_lim.hip")).read()
    assert len(pkg._abi.WEIGHTS_EXPORTS) == 3      # a list of its own: the other lists keep their lengths


def test_bind_limits_refuses_a_library_without_it(oracle_lib):
    with pytest.raises(RuntimeError):
        pkg._abi.bind_limits(oracle_lib)


def test_argument_rules(lim_emu):
    """Every EINVAL / ENOTSUP rule of the header, through the functions the library calls (limits.hpp; no GPU needed)."""
    _, raw = lim_emu
    ok = np.tile(np.array([12.0, -0.3, -1.2, 1.8, 0.3, -0.8, 2.2, 0.1, 0.4, -3.0, 3.0, np.nan]), (5, 1))

    def cs(b0=0, nb=5, rows=ok, dev=0, f32=0, batch=5):
        return raw.lim_emu_check_set(batch, 3, f32, b0, nb, None if rows is None else rows.ctypes.data, dev)
    assert cs() == 0 and cs(b0=2, nb=3) == 0 and cs(b0=4, nb=1) == 0 and cs(rows=np.full((5, 12), np.nan)) == 0
    for kw in (dict(b0=-1), dict(b0=5, nb=1), dict(nb=0), dict(nb=-2), dict(b0=1, nb=5), dict(nb=6), dict(rows=None), dict(rows=None, dev=1)):
        assert cs(**kw) == EINVAL, kw
    for e in range(12):
        for bad in (np.inf, -np.inf):
            a = ok.copy(); a[3, e] = bad
            assert cs(rows=a) == (0 if e == lc.PAD else EINVAL), (e, bad)
            assert cs(rows=a, dev=1) == 0 and cs(rows=a, nb=3) == 0      # a device source is not read; rows behind nb are not either
        a = ok.copy(); a[3, e] = np.nan
        assert cs(rows=a) == 0, e      # NaN: unset
    for e, bad in ((lc.TORQUE, 0.0), (lc.TORQUE, -1.0), (lc.MU, 0.0), (lc.MU, -0.2), (lc.JLB, 0.3), (lc.JLB + 1, 0.0), (lc.JUB + 2, 1.8), (lc.JSLB, 3.0), (lc.JSUB, -3.5)):
        a = ok.copy(); a[2, e] = bad
        assert cs(rows=a) == EINVAL, (e, bad)
    a = ok.copy(); a[2, lc.JLB] = 5.0; a[2, lc.JUB] = np.nan
    assert cs(rows=a) == 0      # one of a pair: nothing to compare it with
    assert cs(f32=1) == ENOTSUP and raw.lim_emu_check_get(5, 3, 1, 0, 0, 5) == ENOTSUP
    assert raw.lim_emu_check_get(5, 3, 0, 0, 0, 5) == 0 and raw.lim_emu_check_get(5, 3, 0, 2, 3, 2) == 0
    for args in ((5, 3, 0, 3, 0, 5), (5, 3, 0, -1, 0, 5), (5, 3, 0, 0, 3, 3), (5, 3, 0, 0, 0, 0)):
        assert raw.lim_emu_check_get(*args) == EINVAL, args
    assert raw.lim_emu_check_kappa(1.0) == 0 and raw.lim_emu_check_kappa(0.3) == 0
    for k in (0.0, -0.1, 1.0 + 1e-12, np.nan, np.inf):
        assert raw.lim_emu_check_kappa(k) == EINVAL, k


def test_rules_and_loops_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/cpp/limits_rules.cpp: a stand-alone program over the same pure host header, built with -fsanitize=address,undefined and run on its own."""
    exe = tmp_path / "limits_rules"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "limits_rules.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
    assert int(r.stdout.split()[1]) > 1000


def test_launch_rule_matches_its_transcription_and_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/roll_pick_table.cpp, a stand-alone program around the rule that picks the rollout and LQ kernels of a launch
    (cafe-mpc_amd/csrc/roll_pick.hpp): all 2^10 switch settings field by field against a transcription of the branches the launch helpers had before,
    exactly the eleven + four kernels reachable, the six kernels of before without tables and heights, the inert combinations inert, the timing suffix
    the kernel's.  Compiled with -fsanitize=address,undefined and run directly; it has to finish clean."""
    exe = str(tmp_path / "roll_pick_table")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "roll_pick_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "roll_pick_table: clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _resources(text):
    """{kernel: {key: int}} of a -Rpass-analysis=kernel-resource-usage listing."""
    t, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            mm = re.match(r"_Z(?:N2hs)?(\d+)(.*)", m.group(1)[len("Function Name: "):])      # the length in front of a mangled name says where it ends
            name = mm.group(2)[:int(mm.group(1))]; t[name] = {}
        else:
            k, v = m.group(1).rsplit(":", 1); t[name][k.strip()] = int(v)
    return t


TWINS = {"k_rollout_lim": "k_rollout", "k_rollout_quad_lim": "k_rollout_quad", "k_lq_lim": "k_lq"}


def test_make_resources_lim():
    """make resources-lim lists exactly the new kernels; each _lim kernel runs at its twin's waves per SIMD and LDS size (the twins' figures: `make
    resources` as profiles/r18pw_kernel_resource_usage.txt recorded it) and none has scratch; the committed record is this build's."""
    out = _resources(subprocess.run(["make", "-C", CSRC, "resources-lim"], capture_output=True, text=True, check=True).stdout)
    assert sorted(out) == sorted(list(TWINS) + ["k_pack_limits", "k_lim_mu"])
    twins = _resources(open(os.path.join(ROOT, "profiles", "r18pw_kernel_resource_usage.txt")).read())
    rec = _resources(open(os.path.join(ROOT, "profiles", "r19lim_kernel_resource_usage.txt")).read())
    for k, twin in TWINS.items():
        print(f"[limits] {k}: {out[k]}\n[limits]   twin {twin}: {twins[twin]}")
        assert out[k]["Occupancy [waves/SIMD]"] == twins[twin]["Occupancy [waves/SIMD]"], k
        assert out[k]["LDS Size [bytes/block]"] == twins[twin]["LDS Size [bytes/block]"], k
    for k in out:
        assert out[k]["ScratchSize [bytes/lane]"] == 0, k
        assert out[k] == rec[k], k
    assert out["k_pack_limits"]["LDS Size [bytes/block]"] == 0 and out["k_lim_mu"]["LDS Size [bytes/block]"] == 0


def test_the_one_command_build_guard_and_the_resources_target():
    """hsddp_hip.hip leaves hsddp_lim.hip out under -DHS_LIM_SEPARATE and under -DHS_PW_SEPARATE (the flag list tests/test_weights_host.py compiles it
    with does not know the newer switch); `make resources` does not compile hsddp_lim.hip."""
    text = open(os.path.join(CSRC, "hsddp_hip.hip")).read()
    assert re.search(r"#if !defined\(HS_LIM_SEPARATE\) && !defined\(HS_PW_SEPARATE\)\n#include \"hsddp_lim.hip\"", text)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    res = re.search(r"^resources: .*\n\t(.*)$", mk, flags=re.M).group(1)
    assert "hsddp_lim.hip" not in res and "build/hsddp_lim.o" in mk and "-DHS_LIM_SEPARATE -c hsddp_lim.hip" in mk


def test_multiphase_ddp_header_compiles_with_limits(tmp_path):
    src = tmp_path / "l.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, hsddp::Episode& e) {\n'
                   '    std::vector<double> rows(2 * HSDDP_LIMITS_ROW, 1.0);\n'
                   '    bool ok = s.set_limits(rows.data(), 2) && s.set_limits(rows.data(), 2, 0, true) && s.limits(rows.data(), 0, 0, 2) && s.clear_limits() && e.plan_friction(0.7);\n'
                   '    (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "l.o")])
