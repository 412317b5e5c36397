"""CPU tests of per-problem touchdown heights (include/hsddp_touchdown.h).

1. Both terminal programs with heights, by value, under the lane emulator (tests/_emu/tdh_emu.cpp): the schedules and the preparation of
   tests/test_quad_terminal_host.py, heights that differ per problem and between the feet of one touchdown.  With ground_height = 0 the stored
   constraint value is the one without heights minus the height BIT FOR BIT (x - 0.0 is exact, both are fpos.z - g); Phi - Phibase is the AL sum
   over the touchdown feet in foot order within 1e-13 x scale (the same few products, possibly contracted differently by the compiler); the quad
   program matches the one-wave program within that file's 1e-11; probes leave every record untouched.
2. Heights equal to the shared value everywhere: every output equals the evaluation without heights within 1e-13 x scale.
3. k_td_terrain's host build against problems.touchdown_heights_from_terrain, bit for bit.
4. The ABI (header against the ctypes mirror, exports) and the argument rules; the stand-alone walk of the rules under AddressSanitizer and UBSan.
5. make resources-tdh.
6. The C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import touchdown_common as tdc

RTOL = 1e-11      # quad program against the one-wave program (tests/test_quad_terminal_host.py)
CASES = {
    "two_foot_touchdown": dict(schedule=((1, 0, 0, 1), (0, 1, 1, 0)), horizons=(2, 3), last_next=(1, 0, 0, 1)),
    "four_foot_touchdown_after_flight": dict(schedule=((1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1)), horizons=(1, 2, 3), last_next=(1, 1, 1, 1)),
}
CSRC = os.path.join(ROOT, "cafe-mpc_amd", "csrc")


@pytest.fixture(scope="module")
def tdh_emu(tmp_path_factory):
    return tdc.build_emu(tmp_path_factory.mktemp("tdh_emu"))


def _close(tag, a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), tag
    m = ~np.isnan(a)
    if not m.any():
        return
    err = np.abs(a[m] - b[m]).max(); sc = max(1.0, np.abs(a[m]).max())
    assert err <= rtol * sc, f"{tag}: |diff| = {err:.3e} > {rtol * sc:.3e} (scale {sc:.3e})"


def _prepared(lib, raw, phases, x0, opt):
    s = pkg.Solver(lib, phases, batch=x0.shape[0])
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    s.hybrid_rollout(0.0, opt); s.update_nominal_trajectory(); s.LQ_approximation(opt)
    assert s.backward_sweep(0.0).all()
    s.linear_rollout(1.0, opt)
    for i in range(len(phases)):
        raw.term_emu_set_al(s.h, i, 10.0, 0.75, 0.3, -0.04)
    return s


@pytest.mark.parametrize("batch", [1, 3, 17])
@pytest.mark.parametrize("case", sorted(CASES))
def test_both_terminal_programs_with_heights_by_value(tdh_emu, case, batch):
    lib, raw = tdh_emu
    phases = pkg.problems.wb_trot_problem(**CASES[case])
    nph = len(phases)
    assert all(p["desc"].ground_height == 0.0 for p in phases)
    legs = tdc.td_legs(phases)
    x0 = pkg.problems.wb_ensemble_x0(batch, 20241222)
    opt0 = pkg.mhpc_ddp_setting()
    hts = tdc.mixed_heights(batch, nph)
    for i in range(nph):      # the heights differ between the feet of one touchdown and between problems
        if legs[i].sum() >= 2:
            assert (np.ptp(hts[:, i][:, legs[i]], axis=1) > 0).all()
        if batch > 1 and legs[i].any():
            assert (np.ptp(hts[:, i][:, legs[i]], axis=0) > 0).all()
    # four handles in the same state: one-wave / quad, without / with heights
    s0w, s0q, shw, shq = (_prepared(lib, raw, phases, x0, opt0) for _ in range(4))
    steps = {"1": np.ones(batch), "0.25": np.full(batch, 0.25), "from_state": 0.5 ** np.arange(batch)}
    for al in (1, 0):
        opt = pkg.mhpc_ddp_setting(AL_active=al)
        for name, eps in steps.items():
            tag = f"{case} B={batch} AL={al} eps={name}"
            for prog, s in ((tdc.WAVE, shw), (tdc.QUAD, shq)):      # probes leave every record untouched
                before = tdc.state(raw, s)
                tdc.terminal(raw, s, prog, eps, opt, False, hts)
                after = tdc.state(raw, s)
                for i in range(nph):
                    for k in before[i]:
                        assert np.array_equal(before[i][k], after[i][k], equal_nan=True), (tag, "probe wrote", prog, i, k)
            pw, pq = tdc.terminal(raw, shw, tdc.WAVE, eps, opt, False, hts), tdc.terminal(raw, shq, tdc.QUAD, eps, opt, False, hts)
            o0w, o0q = tdc.terminal(raw, s0w, tdc.WAVE, eps, opt, True), tdc.terminal(raw, s0q, tdc.QUAD, eps, opt, True)
            ohw, ohq = tdc.terminal(raw, shw, tdc.WAVE, eps, opt, True, hts), tdc.terminal(raw, shq, tdc.QUAD, eps, opt, True, hts)
            assert np.array_equal(pw, ohw) and np.array_equal(pq, ohq), tag      # writing does not change what a program returns
            for q, what in enumerate(("cost", "dsq", "maxh", "ming")):
                _close(f"{tag} quad vs wave {what}", ohw[..., q], ohq[..., q], RTOL)
            for prog, s0, sh, o0, oh in (("wave", s0w, shw, o0w, ohw), ("quad", s0q, shq, o0q, ohq)):
                a, b = tdc.state(raw, s0), tdc.state(raw, sh)
                for i in range(nph):
                    nt = int(legs[i].sum())
                    th0, thh = a[i]["REC"][:, 2:], b[i]["REC"][:, 2:]
                    want = th0.copy(); want[:, :nt] = th0[:, :nt] - hts[:, i][:, legs[i]]
                    assert np.array_equal(thh, want, equal_nan=True), (tag, prog, i, "th is not th0 - height bit for bit")
                    assert np.array_equal(a[i]["REC"][:, 0], b[i]["REC"][:, 0]), (tag, prog, i, "Phibase moved")      # the cost without the AL terms does not see the heights
                    sg, lm = tdc.al_params(raw, sh, i)
                    c = tdc.al_sum(thh, sg, lm, nt) if al else np.zeros(batch)
                    d = b[i]["REC"][:, 1] - b[i]["REC"][:, 0]
                    sc = max(1.0, np.abs(b[i]["REC"][:, 1]).max())
                    assert np.abs(d - c).max() <= 1e-13 * sc, (tag, prog, i, np.abs(d - c).max())
                    if nt:
                        assert np.array_equal(oh[:, i, 2], np.abs(thh[:, :nt]).max(axis=1)), (tag, prog, i, "max |h|")
                    # the state, the reset map and the defects do not depend on the heights
                    assert np.array_equal(a[i]["X"], b[i]["X"]) and np.array_equal(a[i]["XSIM"], b[i]["XSIM"]) and np.array_equal(a[i]["DEFECT"], b[i]["DEFECT"]), (tag, prog, i)
                    assert np.array_equal(o0[:, i, 1], oh[:, i, 1]), (tag, prog, i)
            if al == 1 and name == "1":      # the heights are seen: the constraint values moved by them
                for i in range(nph):
                    if legs[i].any():
                        assert np.abs(tdc.records(raw, shq, i)[:, 2] - tdc.records(raw, s0q, i)[:, 2]).max() > 1e-4, (tag, i)
    for s in (s0w, s0q, shw, shq):
        s.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_heights_equal_to_the_shared_value_change_nothing(tdh_emu, case):
    lib, raw = tdh_emu
    batch = 3
    phases = pkg.problems.wb_trot_problem(**CASES[case])
    nph = len(phases)
    x0 = pkg.problems.wb_ensemble_x0(batch, 20241222)
    opt = pkg.mhpc_ddp_setting()
    shared = np.zeros((batch, nph, 4)) + np.array([p["desc"].ground_height for p in phases])[None, :, None]
    for prog in (tdc.WAVE, tdc.QUAD):
        s0, sh = (_prepared(lib, raw, phases, x0, opt) for _ in range(2))
        for eps in (np.ones(batch), np.full(batch, 0.25)):
            o0, oh = tdc.terminal(raw, s0, prog, eps, opt, True), tdc.terminal(raw, sh, prog, eps, opt, True, shared)
            _close(f"{case} {prog} partials", o0, oh, 1e-13)
            a, b = tdc.state(raw, s0), tdc.state(raw, sh)
            for i in range(nph):
                for k in a[i]:
                    _close(f"{case} {prog} phase {i} {k}", a[i][k], b[i][k], 1e-13)
        s0.close(); sh.close()


@pytest.mark.parametrize("use_map", [True, False])
def test_terrain_lookup_host_build_matches_the_numpy_definition(tdh_emu, use_map):
    """Phase 0 with per-problem references, phase 1 with shared ones, phase 2 without a touchdown (left alone); footholds inside the grid, outside it
    on every side, on its edges, and one NaN."""
    lib, raw = tdh_emu
    B = 17
    phases = pkg.problems.wb_trot_problem(schedule=((1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1)), horizons=(2, 3, 2), last_next=(1, 1, 1, 1))
    legs = tdc.td_legs(phases)
    assert legs[0].any() and legs[1].any() and not legs[2].any()
    ter, mo = tdc.lookup_terrain(), (tdc.lookup_map(B) if use_map else None)
    fp0 = tdc.lookup_footholds(B, 3, 5)
    fp1 = tdc.lookup_footholds(1, 4, 6)[0]
    got = tdc.emu_terrain(raw, ter, mo, 0.0125, B, [fp0, fp1, None])

    class FakeSolver:      # what touchdown_heights_from_terrain reads of a solver
        batch = B

        def get_references(self, i):
            return {"foot_pos": fp0 if i == 0 else np.broadcast_to(fp1, (B,) + fp1.shape)}
    fake = FakeSolver(); fake.phases = phases
    want = pkg.problems.touchdown_heights_from_terrain(fake, ter, mo, 0.0125)
    assert sorted(want) == [0, 1]
    for i in (0, 1):
        assert np.array_equal(got[i], want[i]), i
    assert np.isnan(got[2]).all()
    H = ter.grid()
    m = np.zeros(B, dtype=int) if mo is None else mo
    assert got[0][0, 0] == 0.0125 + H[m[0], np.clip(int(np.floor((fp0[0, -1, 1] + 0.25) / 0.15)), 0, 3), 0]      # x = -5: the first column holds
    assert got[0][1, 1] == 0.0125 + H[m[1], np.clip(int(np.floor((fp0[1, -1, 4] + 0.25) / 0.15)), 0, 3), 4]      # x = 7: the last column holds
    assert got[0][4, 0] == 0.0125 + H[m[4], 3, 0]
    assert got[0][5, 1] == 0.0125 + H[m[5], np.clip(int(np.floor((fp0[5, -1, 4] + 0.25) / 0.15)), 0, 3), 0]      # NaN x reads column 0
    # the shared-reference path of the definition (a list of phase dicts) agrees with the solver path
    flat = pkg.problems.touchdown_heights_from_terrain(phases, ter, mo, 0.0, batch=B)
    assert sorted(flat) == [0, 1] and flat[0].shape == (B, 4)


def test_header_matches_the_ctypes_mirror_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "hsddp_touchdown.h")).read()
    protos = dict(re.findall(r"^int (hsddp_\w+)\((.*?)\);", text, flags=re.M))
    assert sorted(protos) == sorted(pkg._abi.TOUCHDOWN_EXPORTS)
    lib = pkg._abi.bind_touchdown(C.CDLL(os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")))
    for name, args in protos.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(args.split(",")), name
        for ct, decl in zip(fn.argtypes, args.split(",")):
            decl = decl.strip()
            if "*" in decl:
                assert ct in (C.c_void_p, C.POINTER(pkg._abi.TerrainParams)), (name, decl)
            else:
                assert ct is (C.c_double if decl.startswith("double") else C.c_int), (name, decl)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so")], capture_output=True, text=True, check=True).stdout
    for name in pkg._abi.TOUCHDOWN_EXPORTS:
        assert re.search(rf" T {name}$", nm, flags=re.M), name
    assert "terrain-aware planning (the solver does not see the grid)" not in open(os.path.join(ROOT, "include", "hsddp_terrain.h")).read()


def test_bind_touchdown_refuses_a_library_without_it(oracle_lib):
    with pytest.raises(RuntimeError):
        pkg._abi.bind_touchdown(oracle_lib)


def test_argument_rules(tdh_emu):
    """Every EINVAL / ENOTSUP rule of the header, through the functions the library calls (touchdown.hpp; no GPU needed)."""
    lib, raw = tdh_emu
    EINVAL, ENOTSUP = -1, -4
    model = np.array([0, 0, 1, 2], dtype=np.int32); nt = np.array([2, 0, 0, 0], dtype=np.int32)
    ok = np.full((5, 4), 0.02)

    def cs(phase=0, b0=0, nb=5, heights=ok, dev=0, f32=0):
        return raw.tdh_emu_check_set(4, 5, f32, model.ctypes.data_as(tdc.IP), nt.ctypes.data_as(tdc.IP), phase, b0, nb, None if heights is None else heights.ctypes.data, dev)
    assert cs() == 0 and cs(b0=2, nb=3) == 0
    for kw in (dict(phase=-1), dict(phase=4), dict(b0=-1), dict(nb=0), dict(nb=-2), dict(b0=1, nb=5), dict(nb=6), dict(heights=None), dict(phase=1)):
        assert cs(**kw) == EINVAL, kw
    for bad in (np.nan, np.inf, -np.inf):
        a = ok.copy(); a[3, 2] = bad
        assert cs(heights=a) == EINVAL and cs(heights=a, dev=1) == 0 and cs(heights=a, nb=3) == 0
    assert cs(phase=2) == ENOTSUP and cs(phase=3) == ENOTSUP and cs(f32=1) == ENOTSUP
    H = np.zeros((3, 4, 5)); mo = np.array([0, 1, 2, 1, 0], dtype=np.int32)

    def ct(nx=5, ny=4, nm=3, x0=0.0, y0=0.0, cx=0.1, cy=0.1, zg=0.0, H=H, mo=mo, dev=0, f32=0):
        return raw.tdh_emu_check_terrain(5, f32, nx, ny, nm, x0, y0, cx, cy, zg, None if H is None else H.ctypes.data, None if mo is None else mo.ctypes.data, dev)
    assert ct() == 0 and ct(mo=None) == 0
    Hn = H.copy(); Hn[2, 3, 4] = np.nan
    mb = mo.copy(); mb[4] = 3
    for kw in (dict(H=None), dict(x0=np.nan), dict(y0=np.inf), dict(cx=0.0), dict(cy=-1.0), dict(cx=np.nan), dict(zg=np.nan), dict(nx=0), dict(ny=0), dict(nm=0),
               dict(nx=1025, dev=1), dict(ny=1025, dev=1), dict(nm=4097, dev=1), dict(nx=1024, ny=1024, nm=5, dev=1), dict(H=Hn), dict(mo=mb), dict(mo=-mo - 1)):
        assert ct(**kw) == EINVAL, kw
    assert ct(f32=1) == ENOTSUP


def test_rules_and_lookup_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/cpp/touchdown_table.cpp: a stand-alone program over the same pure host header, built with -fsanitize=address,undefined and run on its own."""
    exe = tmp_path / "touchdown_table"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "touchdown_table.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
    assert int(r.stdout.split()[1]) > 100


def test_make_resources_tdh_lists_the_new_kernels_at_their_limits():
    """make resources-tdh lists exactly the new kernels.  The quad variant: the limits of tests/test_quad_terminal_resources.py (no scratch, at most
    40 KiB of LDS, one wave per SIMD); the one-wave variant: k_rollout's occupancy, as make resources recorded it.  Registers and spills are printed
    (DESIGN.md records them), not asserted."""
    out = subprocess.run(["make", "-C", CSRC, "resources-tdh"], capture_output=True, text=True, check=True).stdout
    t, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            name = m.group(1)[len("Function Name: "):]; t[name] = []
        else:
            t[name].append(m.group(1))
    short = {re.match(r"_Z\d+(k_[a-z_0-9]+)", k).group(1): v for k, v in t.items()}

    def strip(n):      # the mangled name runs into the first parameter's code
        for want in ("k_rollout_quad_term_tdh", "k_rollout_tdh", "k_td_terrain"):
            if n.startswith(want):
                return want
        return n
    short = {strip(k): v for k, v in short.items()}
    assert sorted(short) == ["k_rollout_quad_term_tdh", "k_rollout_tdh", "k_td_terrain"]
    for k, v in short.items():
        print("[tdh]", k, "; ".join(v))

    def val(k, key):
        return int(next(x for x in short[k] if x.startswith(key)).split(":")[1])
    assert val("k_rollout_quad_term_tdh", "ScratchSize") == 0
    assert val("k_rollout_quad_term_tdh", "LDS Size") <= 40 * 1024
    assert val("k_rollout_quad_term_tdh", "Occupancy") == 1
    parent = open(os.path.join(ROOT, "profiles", "r11uni_kernel_resource_usage_parent.txt")).read()
    m = re.search(r"Function Name: _Z9k_rolloutPK.*?Occupancy \[waves/SIMD\]: (\d+)", parent, flags=re.S)
    assert m and val("k_rollout_tdh", "Occupancy") == int(m.group(1))
    assert val("k_td_terrain", "ScratchSize") == 0 and val("k_td_terrain", "LDS Size") == 0


def test_multiphase_ddp_header_compiles_with_touchdown(tmp_path):
    """The C++ mirror: set_touchdown_heights / touchdown / clear_touchdown_heights / plan_terrain and Episode::plan_terrain compile."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const hsddp_terrain_t& t, const double* H, const int* map_of) {\n'
                   '    std::vector<double> hts(8), val(8);\n'
                   '    bool ok = s.set_touchdown_heights(1, hts.data(), 2) && s.set_touchdown_heights(1, hts.data(), 2, 0, true) && s.touchdown(1, hts.data(), val.data(), 0, 2)\n'
                   '              && s.plan_terrain(t, H, map_of, 0.0) && s.plan_terrain(t, H) && s.clear_touchdown_heights(1) && s.clear_touchdown_heights();\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.plan_terrain(); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
