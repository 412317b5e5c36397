"""Per-problem cost-weight scales (include/hsddp_weights.h) without a GPU: the scaled whole-body programs under the lane emulator
(tests/_emu/pw_emu.cpp; both programs: the one-wave knots and the lane quad), the packing loop, the ABI and the build.

The reference is tests/pw_common.StackedOracle: B single-problem oracle handles whose descriptors carry q * sq_b, r * sr_b, qf * sqf_b.

1. test_inputs_qualify / test_scaled_programs_match_the_stacked_oracle: per-iterate parity at parity_common's plain tolerances (rtol 1e-8, K 1e-6
   absolute, two iterates, no arbiter) on the three cases of pw_common.CASES with B = 1, 5, 17; every input first qualifies with the long-double oracle
   at 0.05 x those tolerances.  On the MHPC case the single-rigid-body fields equal those of a run without scales bit for bit.
2. test_unit_scales_are_the_unscaled_programs: rows of 1.0 against no table, within the plain tolerances; the measured difference is printed.
3. test_pack_host_build_matches_numpy: k_pack_weights' loop bit for bit - first call, later ranges, a device-style source.
4. ABI: the header against the ctypes mirror, every refusal rule, the rules and the loop as a stand-alone program under ASan + UBSan.
5. test_make_resources_pw: every _pw kernel at its twin's waves per SIMD and LDS size; registers, spills and scratch are printed beside the twin's.
6. Build: the C++ mirror compiles; the gfx950 code objects of every translation unit the parent has keep their .text, .rodata and symbol list
   (nine units across the change that added the scales; all eleven across the one that wrote the launch rule down in roll_pick.hpp).

Real HIP execution: tests/test_weights_gpu.py."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import parity_common as pc
import pattern_common as pt
import pw_common as pw
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "cafe-mpc_amd", "csrc")
QUALIFY = 0.05
PROGRAMS = {"wave": pw.WAVE, "quad": pw.QUAD}


@pytest.fixture(scope="module")
def pw_emu(tmp_path_factory):
    return pw.build_emu(tmp_path_factory.mktemp("pw_emu"))


def _x0(case, batch):
    return pkg.problems.wb_ensemble_x0(batch, pw.CASES[case][1])


@pytest.mark.parametrize("case", list(pw.CASES))
def test_inputs_qualify(oracle_lib, oracle_ld_lib, case):
    """B = 17 holds the problems of B = 1 and B = 5 (same seeds, the first rows): one qualification serves every batch."""
    phases = pw.CASES[case][0](); x0 = _x0(case, 17); rows = pw.scale_rows(17)
    assert np.array_equal(_x0(case, 5), x0[:5]) and np.array_equal(pw.scale_rows(5), rows[:5]) and np.all(rows[0] == 1.0)
    assert rows[1:].min() >= 0.25 and rows[1:].max() <= 4.0 and len({r.tobytes() for r in rows}) == 17
    so, sx = pw.StackedOracle(oracle_lib, phases, x0, rows), pw.StackedOracle(oracle_ld_lib, phases, x0, rows)
    report = pc.run_steps(pkg, so, sx, phases, pkg.mhpc_ddp_setting(), n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
    print(f"[weights] qualify {case}: oracle-vs-long-double / (0.05 x tolerance) {pt.worst_ratio(report)}")
    so.close(); sx.close()


@pytest.mark.parametrize("program", list(PROGRAMS))
@pytest.mark.parametrize("batch", pw.BATCHES)
@pytest.mark.parametrize("case", list(pw.CASES))
def test_scaled_programs_match_the_stacked_oracle(pw_emu, oracle_lib, case, batch, program):
    lib, raw = pw_emu
    phases = pw.CASES[case][0](); x0 = _x0(case, batch); rows = pw.scale_rows(batch)
    so = pw.StackedOracle(oracle_lib, phases, x0, rows)
    se = pw.PwEmu(lib, raw, phases, x0, rows, PROGRAMS[program])
    report = pc.run_steps(pkg, so, se, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    print(f"[weights] {case} B={batch} {program}: error / tolerance {pt.worst_ratio(report)}")
    so.close(); se.close()


@pytest.mark.parametrize("program", list(PROGRAMS))
def test_reduced_model_phases_do_not_see_the_scales(pw_emu, program):
    """MHPC case: rollout, LQ approximation and backward sweep from the same state - the single-rigid-body phase's fields are those of a run without
    scales bit for bit (its knots read no row, and the sweep reaches it before any whole-body knot), while the whole-body fields differ."""
    lib, raw = pw_emu
    phases = pw.CASES["mhpc"][0](); x0 = _x0("mhpc", 5); rows = pw.scale_rows(5); opt = pkg.mhpc_ddp_setting()
    runs = [pw.PwEmu(lib, raw, phases, x0, r, PROGRAMS[program]) for r in (rows, None)]
    for s in runs:
        s.hybrid_rollout(0.0, opt); s.compute_cost(opt); s.update_nominal_trajectory(); s.LQ_approximation(opt); assert s.backward_sweep(0.0).all()
    srb = [i for i, p in enumerate(phases) if p["desc"].model != pw.MODEL_WB]
    assert srb
    for i in srb:
        for f in pc.STEP_FIELDS["rollout"] + pc.STEP_FIELDS["lq"] + pc.STEP_FIELDS["sweep"]:
            a, b = runs[0].field(i, f), runs[1].field(i, f)
            assert np.array_equal(a, b), (i, f)
    assert not np.array_equal(runs[0].field(0, "LXX")[1:], runs[1].field(0, "LXX")[1:])      # (row 0 is all ones)
    for s in runs:
        s.close()


@pytest.mark.parametrize("program", list(PROGRAMS))
@pytest.mark.parametrize("case", list(pw.CASES))
def test_unit_scales_are_the_unscaled_programs(pw_emu, case, program, monkeypatch):
    """Rows of 1.0 set explicitly against no table: one rollout + LQ evaluation from the same state and two iterates, within the plain tolerances.
    q * 1.0 is q, so the difference is expected at rounding level (the scaled program is another instantiation: bit equality is not promised)."""
    lib, raw = pw_emu
    phases = pw.CASES[case][0](); x0 = _x0(case, 5)
    if program == "quad":      # the unscaled lane-quad knot is emu.cpp's, behind its environment switch
        monkeypatch.setenv("HSDDP_EMU_QUAD", "1")
    else:
        monkeypatch.delenv("HSDDP_EMU_QUAD", raising=False)
    sa = pw.PwEmu(lib, raw, phases, x0, None, PROGRAMS[program])
    sb = pw.PwEmu(lib, raw, phases, x0, np.ones((5, pw.ROW)), PROGRAMS[program])
    report = pc.run_steps(pkg, sa, sb, phases, pkg.mhpc_ddp_setting(), n_iter=2)
    first = max(v[0] / v[3] for k, v in report.items() if k[0] in ("rollout0", "lq0"))
    print(f"[weights] unit scales {case} {program}: first rollout + LQ error / tolerance {first:.3e}; two iterates {pt.worst_ratio(report)}; "
          f"largest absolute difference {max(v[0] for v in report.values()):.3e}")
    sa.close(); sb.close()


def test_pack_host_build_matches_numpy(pw_emu):
    _, raw = pw_emu
    B = 17
    r = np.random.default_rng(5)
    table = np.full((B, pw.ROW), -7.0); want = np.ones((B, pw.ROW))
    src = r.uniform(0.25, 4.0, size=(5, pw.ROW))
    raw.pw_emu_pack(table.ctypes.data_as(pw.DP), B, src.ctypes.data_as(pw.DP), 3, 5, 1)      # first call: 1.0 everywhere, then rows 3..7
    want[3:8] = src
    assert np.array_equal(table, want)
    for b0, nb in ((0, 1), (16, 1), (7, 10), (0, 17)):      # later calls overwrite their range only (the source is any [nb][84] block: device-style too)
        src = np.ascontiguousarray(r.uniform(0.25, 4.0, size=(nb + 2, pw.ROW))[1:-1])
        raw.pw_emu_pack(table.ctypes.data_as(pw.DP), B, src.ctypes.data_as(pw.DP), b0, nb, 0)
        want[b0:b0 + nb] = src
        assert np.array_equal(table, want), (b0, nb)
    rows = pkg._abi.pack_weight_scales(np.full(36, 2.0), np.full(12, 3.0), np.arange(36.0), nb=4)      # broadcasting from one row
    assert rows.shape == (4, 84) and np.all(rows[:, :36] == 2.0) and np.all(rows[:, 36:48] == 3.0) and np.array_equal(rows[2, 48:], np.arange(36.0))
    with pytest.raises(ValueError):
        pkg._abi.pack_weight_scales(np.ones(35), np.ones(12), np.ones(36))


def test_header_matches_the_ctypes_mirror_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "hsddp_weights.h")).read()
    protos = dict(re.findall(r"^int (hsddp_\w+)\((.*?)\);", text, flags=re.M))
    assert sorted(protos) == sorted(pkg._abi.WEIGHTS_EXPORTS)
    assert int(re.search(r"#define HSDDP_WEIGHTS_ROW (\d+)", text).group(1)) == pkg._abi.WEIGHTS_ROW == pw.ROW
    lib = pkg._abi.bind_weights(C.CDLL(os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")))
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(args.split(",")), name
        for ct, decl in zip(fn.argtypes, args.split(",")):
            assert ct is (C.c_void_p if "*" in decl else C.c_int), (name, decl)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")], capture_output=True, text=True, check=True).stdout
    for name in pkg._abi.WEIGHTS_EXPORTS:
        assert re.search(rf" T {name}$", nm, flags=re.M), name
    assert "track_cost" in text and "yardstick" in text      # the header says that the episode's track_cost keeps the descriptor's weights


def test_bind_weights_refuses_a_library_without_it(oracle_lib):
    with pytest.raises(RuntimeError):
        pkg._abi.bind_weights(oracle_lib)


def test_argument_rules(pw_emu):
    """Every EINVAL / ENOTSUP rule of the header, through the functions the library calls (weights.hpp; no GPU needed)."""
    _, raw = pw_emu
    EINVAL, ENOTSUP = -1, -4
    ok = np.full((5, pw.ROW), 1.5)

    def cs(b0=0, nb=5, rows=ok, dev=0, f32=0, batch=5):
        return raw.pw_emu_check_set(batch, f32, b0, nb, None if rows is None else rows.ctypes.data, dev)
    assert cs() == 0 and cs(b0=2, nb=3) == 0 and cs(b0=4, nb=1) == 0
    for kw in (dict(b0=-1), dict(b0=5, nb=1), dict(nb=0), dict(nb=-2), dict(b0=1, nb=5), dict(nb=6), dict(rows=None), dict(rows=None, dev=1)):
        assert cs(**kw) == EINVAL, kw
    for e in (0, 35, 36, 47, 48, 83):
        for bad in (np.nan, np.inf, -np.inf, -0.5):
            a = ok.copy(); a[3, e] = bad
            assert cs(rows=a) == EINVAL, (e, bad)
            assert cs(rows=a, dev=1) == 0 and cs(rows=a, nb=3) == 0      # a device source is not read; rows behind nb are not either
        a = ok.copy(); a[3, e] = 0.0
        assert cs(rows=a) == (EINVAL if 36 <= e < 48 else 0), e      # sq, sqf >= 0; sr > 0
    assert cs(f32=1) == ENOTSUP and raw.pw_emu_check_range(5, 1, 0, 5) == ENOTSUP
    assert raw.pw_emu_check_range(5, 0, 0, 5) == 0 and raw.pw_emu_check_range(5, 0, 3, 3) == EINVAL and raw.pw_emu_check_range(5, 0, 0, 0) == EINVAL


def test_rules_and_pack_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/cpp/weights_rules.cpp: a stand-alone program over the same pure host header, built with -fsanitize=address,undefined and run on its own."""
    exe = tmp_path / "weights_rules"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "weights_rules.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
    assert int(r.stdout.split()[1]) > 1000


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


TWINS = {"k_rollout_pw": "k_rollout", "k_rollout_quad_pw": "k_rollout_quad", "k_rollout_quad_term_pw": "k_rollout_quad_term", "k_lq_pw": "k_lq"}


def test_make_resources_pw():
    """make resources-pw lists exactly the new kernels; each runs at its twin's waves per SIMD and LDS size (the twins' figures: `make resources` as
    profiles/r18pw_kernel_resource_usage.txt recorded it).  Registers, spills and scratch are printed beside the twin's (DESIGN.md records them)."""
    out = _resources(subprocess.run(["make", "-C", CSRC, "resources-pw"], capture_output=True, text=True, check=True).stdout)
    assert sorted(out) == sorted(list(TWINS) + ["k_pack_weights"])
    rec = _resources(open(os.path.join(ROOT, "profiles", "r18pw_kernel_resource_usage.txt")).read())
    for k, twin in TWINS.items():
        print(f"[weights] {k}: {out[k]}\n[weights]   twin {twin}: {rec[twin]}")
        assert out[k]["Occupancy [waves/SIMD]"] == rec[twin]["Occupancy [waves/SIMD]"], k
        assert out[k]["LDS Size [bytes/block]"] == rec[twin]["LDS Size [bytes/block]"], k
        assert out[k] == rec[k], k      # the committed record is this build's
    assert out["k_pack_weights"]["ScratchSize [bytes/lane]"] == 0 and out["k_pack_weights"]["LDS Size [bytes/block]"] == 0


def test_multiphase_ddp_header_compiles_with_weight_scales(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s) {\n'
                   '    std::vector<double> rows(2 * HSDDP_WEIGHTS_ROW, 1.0);\n'
                   '    bool ok = s.set_weight_scales(rows.data(), 2) && s.set_weight_scales(rows.data(), 2, 0, true) && s.weight_scales(rows.data(), 0, 2) && s.clear_weight_scales();\n'
                   '    (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])


# ---- untouched code objects: the method of profiles/r15lat_section_hashes.txt
HIPCC = "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/llvm/bin"
QUAD_FLAGS = ["-mllvm", "-disable-machine-licm"]
SEPARATE = ["-DHS_QUAD_SEPARATE", "-DHS_SUB_SEPARATE", "-DHS_UNI_SEPARATE", "-DHS_TER_SEPARATE", "-DHS_PLANT_SEPARATE", "-DHS_LAT_SEPARATE", "-DHS_FRIC_SEPARATE", "-DHS_TDH_SEPARATE",
            "-DHS_PW_SEPARATE"]
UNITS = {"hsddp_quad.hip": QUAD_FLAGS, "hsddp_sub.hip": ["-DHS_SUB_SEPARATE"], "hsddp_uni.hip": ["-DHS_UNI_SEPARATE"], "hsddp_ter.hip": ["-DHS_TER_SEPARATE"],
         "hsddp_plant.hip": ["-DHS_PLANT_SEPARATE"], "hsddp_lat.hip": ["-DHS_LAT_SEPARATE"], "hsddp_fric.hip": QUAD_FLAGS + ["-DHS_FRIC_SEPARATE"],
         "hsddp_tdh.hip": QUAD_FLAGS + ["-DHS_TDH_SEPARATE"], "hsddp_hip.hip": SEPARATE}


_HASHED = {}


def section_hashes(unit, flags, tmp, csrc=CSRC):
    """sha256 of .text, .rodata and the symbol list (llvm-readelf -sW without the __hip_cuid_ line and the index column, sorted) of the unit's gfx950
    code object, compiled with the Makefile's flags plus --cuda-device-only -c."""
    import hashlib
    key = (unit, tuple(flags), csrc)
    if key in _HASHED:      # (the two tests below hash the same build: each unit is compiled once)
        return _HASHED[key]
    base = os.path.join(str(tmp), unit)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-Wno-unused-value", "-DROLL_WPE=2", "--cuda-device-only", "-c", *flags,
                           unit, "-o", base + ".bun"], cwd=csrc, stderr=subprocess.DEVNULL)
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + base + ".bun", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + base + ".co"])
    out = {}
    for sec in (".text", ".rodata"):
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", f"{sec}={base}{sec}", base + ".co"])
        out[sec] = hashlib.sha256(open(base + sec, "rb").read()).hexdigest()
    syms = subprocess.run([LLVM + "/llvm-readelf", "-sW", base + ".co"], capture_output=True, text=True, check=True).stdout
    rows = sorted(" ".join(l.split()[1:]) for l in syms.splitlines() if "__hip_cuid_" not in l and len(l.split()) >= 8)
    out[".syms"] = hashlib.sha256("\n".join(rows).encode()).hexdigest()
    _HASHED[key] = out
    return out


def test_code_objects_of_the_parent_s_translation_units_are_untouched(tmp_path):
    """profiles/r18pw_section_hashes.txt holds, per translation unit the parent has, the hashes of the parent commit's code object and of this
    change's; both columns agree there, and this build's code objects still hash to them."""
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "r18pw_section_hashes.txt")):
        if line.startswith("#") or not line.strip():
            continue
        unit, sec, parent, this, verdict = line.split()
        assert parent == this and verdict == "identical", line
        rec[(unit, sec)] = parent
    assert sorted({u for u, _ in rec}) == sorted(UNITS) and len(rec) == 3 * len(UNITS)
    with ThreadPoolExecutor(max_workers=min(len(UNITS), os.cpu_count() or 1, 16)) as ex:
        got = dict(zip(UNITS, ex.map(lambda u: section_hashes(u, UNITS[u], tmp_path), UNITS)))
    for (unit, sec), h in rec.items():
        assert got[unit][sec] == h, (unit, sec)


ALL_UNITS = dict(UNITS, **{"hsddp_pw.hip": QUAD_FLAGS + ["-DHS_PW_SEPARATE"], "hsddp_lim.hip": QUAD_FLAGS + ["-DHS_LIM_SEPARATE"]})


def test_code_objects_of_all_eleven_translation_units_are_untouched_by_the_launch_records(tmp_path):
    """profiles/r20pick_section_hashes.txt: the same record for all eleven translation units across the change that moved the choice of rollout and LQ
    kernel into roll_pick.hpp and the launchers' arguments into records (host code only).  Both columns agree in every row, and this build's code
    objects still hash to them: no kernel's code, constants or symbols moved."""
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "r20pick_section_hashes.txt")):
        if line.startswith("#") or not line.strip():
            continue
        unit, sec, parent, this, verdict = line.split()
        assert parent == this and verdict == "identical", line
        rec[(unit, sec)] = parent
    assert sorted({u for u, _ in rec}) == sorted(ALL_UNITS) and len(ALL_UNITS) == 11 and len(rec) == 3 * len(ALL_UNITS)
    with ThreadPoolExecutor(max_workers=min(len(ALL_UNITS), os.cpu_count() or 1, 16)) as ex:
        got = dict(zip(ALL_UNITS, ex.map(lambda u: section_hashes(u, ALL_UNITS[u], tmp_path), ALL_UNITS)))
    for (unit, sec), h in rec.items():
        assert got[unit][sec] == h, (unit, sec)
