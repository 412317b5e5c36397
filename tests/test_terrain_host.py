"""CPU tests of terrain height maps and early swing-foot touchdown (include/hsddp_terrain.h): the ctypes mirror, the lookup's definition, the reference
walk of tests/ter_common.py, and the program itself (cafe-mpc_amd/csrc/wb_sim.hpp with the TER policies) compiled for the host by tests/_emu/ter_emu.cpp
against that reference - flat ground, a block, a map per sample under noise, feet outside the grid on a partial wave, a contained divergence, and
two ticks with (F, E) handed over.  Plus the amplification through the windows, make resources-ter, a sanitizer run of a stand-alone program around
the host build, and the C++ mirror.  Toggling, the library's refusals and episodes need the library: tests/test_terrain_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc
import mc_common as mc
import grf_common as gc
import uni_common as un
import ter_common as tc

MU = 0.6
EINVAL = -1


def test_terrain_abi_mirror_matches_the_header():
    """Every prototype of include/hsddp_terrain.h is in TERRAIN_EXPORTS and in no other list; bind_terrain refuses a library that lacks one; the row
    dtype and the parameter structure have the layouts of hsddp_terrain_row_t and hsddp_terrain_t; the other lists are what they were."""
    src = open(os.path.join(ROOT, "include", "hsddp_terrain.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = set(re.findall(r"\b(hsddp_terrain_[a-z_]+)\s*\(", code))
    A = pkg._abi
    assert protos == set(A.TERRAIN_EXPORTS) and len(protos) == 3
    others = (set(A.EXPORTS) | set(A.ENSEMBLE_EXPORTS) | set(A.HKD_EXPORTS) | set(A.REFS_EXPORTS) | set(A.SIM_EXPORTS) | set(A.MC_EXPORTS) | set(A.GRF_EXPORTS)
              | set(A.EPISODE_EXPORTS) | set(A.SUBSTEP_EXPORTS) | set(A.CONTACT_EXPORTS))
    assert not protos & others
    assert (len(A.SIM_EXPORTS), len(A.MC_EXPORTS), len(A.GRF_EXPORTS), len(A.EPISODE_EXPORTS), len(A.SUBSTEP_EXPORTS), len(A.CONTACT_EXPORTS)) == (7, 2, 2, 9, 2, 3)

    def members(struct):
        body = re.search(r"typedef struct \{([^{}]*)\} " + struct + ";", code).group(1)
        return [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert members("hsddp_terrain_row_t") == list(A.TERRAIN_ROW_DTYPE.names) and A.TERRAIN_ROW_DTYPE.itemsize == 32 and A.TERRAIN_ROW_DTYPE.fields["max_pen"][1] == 24
    assert members("hsddp_terrain_t") == [f for f, _ in A.TerrainParams._fields_] and ctypes.sizeof(A.TerrainParams) == 56 and A.TerrainParams.x0.offset == 16

    class Fake:
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.CONTACT_EXPORTS + A.TERRAIN_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_terrain(lib)
    setattr(lib, A.TERRAIN_EXPORTS[-1], Fake())
    A.bind_terrain(lib)
    assert len(lib.hsddp_terrain_set.argtypes) == 5 and len(lib.hsddp_terrain_get_params.argtypes) == 3


def test_terrain_height_is_the_clamped_cell():
    """sim.terrain_height: the cell of a point, the edge cell outside the grid on every side, cell 0 for a NaN, the last cell for +inf, a map per point."""
    H = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    t = pkg.sim.Terrain(H=H, x0=-1.0, y0=2.0, cx=0.5, cy=0.25)
    h = lambda p, m=0: pkg.sim.terrain_height(t, np.array(p, dtype=np.float64), m)
    assert h([-1.0, 2.0]) == H[0, 0, 0] and h([-0.5, 2.0]) == H[0, 0, 1] and h([-0.500001, 2.249]) == H[0, 0, 0] and h([0.99, 2.74]) == H[0, 2, 3]
    assert h([-50.0, 2.3]) == H[0, 1, 0] and h([50.0, 2.3]) == H[0, 1, 3] and h([0.1, -9.0]) == H[0, 0, 2] and h([0.1, 9.0]) == H[0, 2, 2]
    assert h([np.nan, np.nan]) == H[0, 0, 0] and h([np.inf, -np.inf], 1) == H[1, 0, 3] and h([1e300, -1e300], 1) == H[1, 0, 3]
    assert np.array_equal(pkg.sim.terrain_height(t, np.array([[0.1, 2.3], [0.1, 2.3]]), np.array([0, 1])), [H[0, 1, 2], H[1, 1, 2]])
    assert pkg.sim.terrain_height(pkg.sim.Terrain(H=np.full((3, 2), 0.5)), np.zeros(2)) == 0.5      # a [ny, nx] array is one map


@pytest.fixture(scope="module")
def ter_emu(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("ter_emu"))


@pytest.fixture(scope="module")
def uni_emu(tmp_path_factory):
    return un.build_emu(tmp_path_factory.mktemp("uni_emu_for_ter"))


@pytest.fixture(scope="module")
def solved_trot(oracle_lib):
    """The fixture of tests/test_contact_host.py: trot 4 x 12, four problems, 3 AL x 4 DDP iterations, eight samples around Xbar[0] (sigma 0.02 / 0.2)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, so, xs, mc.policy_of(so)
    so.close()


@pytest.fixture(scope="module")
def refs():
    """Reference walks shared between the tests of this module (computed once, read only)."""
    return {}


def reference(refs, oracle_lib, solved_trot, case, S):
    phases, so, xs, pol = solved_trot
    if (case, S) not in refs:
        x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
        refs[(case, S)] = tc.oracle_walk_ter(pkg, oracle_lib, phases, pol, sc.step_map(phases, 48), x0, S, fz_rel, zg, ter, d, k)
    return refs[(case, S)]


def test_flat_terrain_on_the_host_is_the_contact_walk(ter_emu, uni_emu, solved_trot):
    """Case 1: H = 0, early = 0, S = 3 on the flight case: the integer rows are those of the program without the terrain, the floats agree within the
    tolerance (whether they are bit-identical is printed), and every new counter is 0."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "flat", xs)
    res = tc.host_run(ter_emu, pkg, so, x0, smap, 3, fz_rel, zg, ter, d, k, MU)
    base = un.host_run(uni_emu, pkg, so, x0, smap, 3, fz_rel, zg, d, k, MU)
    t = res.pop("terrain")
    same = all(res[f].tobytes() == base[f].tobytes() for f in base)
    print(f"[ter] host flat: bit-identical to the program without the terrain: {same}")
    assert base["contact"]["n_release"].sum() > 0 and base["contact"]["n_land"].sum() > 0
    for f in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(res["contact"][f], base["contact"][f]), f
    assert np.array_equal(res["rows"]["first_bad"], base["rows"]["first_bad"]) and np.array_equal(res["grf"]["n_slip"], base["grf"]["n_slip"]) and np.array_equal(res["extra"], base["extra"])
    for f in ("X", "U", "x_final", "Y"):
        sc.close(f"host flat {f}", res[f], base[f], scale=max(1.0, float(np.abs(base[f]).max())))
    sc.close("host flat max_lift", res["contact"]["max_lift"], base["contact"]["max_lift"], scale=1.0)
    assert (t["first_early"] == -1).all() and not t["n_early"].any() and not t["n_early_release"].any() and not t["n_held"].any() and not t["early_final"].any()
    # (max_pen is no counter: it runs over the landing sets T, which hold the stance landings of the contact rule too)
    assert (t["max_pen"] >= 0.0).all() and not t["max_pen"][base["contact"]["n_land"] == 0].any()


def test_reference_walk_on_flat_ground_is_the_contact_reference(oracle_lib, solved_trot):
    """The reference itself: with H = 0 and early = 0 it is uni_common.oracle_walk_uni, bit for bit."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "flat", xs)
    a = tc.oracle_walk_ter(pkg, oracle_lib, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, ter, d, k[:2, 5:])
    b = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, d, k[:2, 5:])
    for f in ("X", "U", "Y", "att", "F", "solves", "force_margin", "kin_margin"):
        assert np.array_equal(a[f], b[f]), f
    assert a["rows"].tobytes() == b["rows"].tobytes() and b["rows"]["n_release"].sum() > 0 and not a["trows"]["n_early"].any()


@pytest.mark.parametrize("case,S", tc.CASES)
def test_program_on_the_host_matches_the_reference(ter_emu, oracle_lib, solved_trot, refs, case, S):
    """Cases 2 - 5 of ter_common.case_setup against the reference walk; the non-vacuity of each case is asserted on the REFERENCE, and so is the cap
    of one left-out sample, before anything is compared.  Then the invariants of the run's own outputs."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
    ref = reference(refs, oracle_lib, solved_trot, case, S)
    tc.assert_case_is_not_vacuous(case, ref, ter)
    res = tc.host_run(ter_emu, pkg, so, x0, smap, S, fz_rel, zg, ter, d, k, MU)
    tc.compare_case(f"host {case} S={S}", pkg, res, ref, mc.xbar_window(pol, smap)[:x0.shape[0]], MU, 0.0, fz_rel)
    fb = gc.force_bound(ref["Y"])
    fin = np.isfinite(res["grf"]["min_fz"])
    assert fin.any() and (res["grf"]["min_fz"][fin] >= fz_rel - fb).all()


def test_a_map_per_sample_on_the_host(ter_emu, oracle_lib, solved_trot, refs):
    """Case 3's own properties: the samples of map 0 equal a one-map run of their own, bit for bit; and, on the reference, the samples of the pit map
    land lower than those of the flat map (ter_common.assert_pit_samples_land_lower)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "maps", xs)
    res = tc.host_run(ter_emu, pkg, so, x0, smap, 4, fz_rel, zg, ter, d, k, MU)
    one = pkg.sim.Terrain(H=ter.grid()[:1], early=True, w_td=ter.w_td)
    alone = tc.host_run(ter_emu, pkg, so, x0, smap, 4, fz_rel, zg, one, d, k, MU)
    m0 = np.asarray(ter.map_of) == 0
    for f in res:
        assert res[f][m0].tobytes() == alone[f][m0].tobytes(), f
    assert not np.array_equal(res["x_final"][~m0], alone["x_final"][~m0])
    ref = reference(refs, oracle_lib, solved_trot, "maps", 4)
    tc.assert_pit_samples_land_lower(ref, ter)


def test_amplification_through_the_terrain_windows(ter_emu, solved_trot):
    """A 1e-12 change of x0 through the 48-step windows of cases 2 and 3 on the host build, over the samples that keep their decisions: printed, and
    at least two orders below the tolerance the windows are held to, 1e-8 x max(1, |X|max) (sim_common.close)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    rng = np.random.default_rng(7)
    for case, S in tc.CASES[:3]:
        x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, case, xs)
        a = tc.host_run(ter_emu, pkg, so, x0, smap, S, fz_rel, zg, ter, d, k, MU)
        b = tc.host_run(ter_emu, pkg, so, x0 + 1e-12 * rng.uniform(-1.0, 1.0, x0.shape), smap, S, fz_rel, zg, ter, d, k, MU)
        same = np.all([a["contact"][f] == b["contact"][f] for f in ("first_release", "n_release", "n_land", "n_free", "free_final")] + [a["terrain"][f] == b["terrain"][f] for f in tc.INTS_T], axis=0)
        assert (a["rows"]["first_bad"] < 0).all() and same.sum() >= same.size - 1
        ev = same & (a["terrain"]["n_early"] > 0)
        amp = np.abs(a["X"][same] - b["X"][same]).max() / 1e-12
        amp_ev = np.abs(a["X"][ev] - b["X"][ev]).max() / 1e-12 if ev.any() else 0.0
        scale = max(1.0, float(np.abs(a["X"]).max()))
        print(f"[ter] amplification {case} S={S}: {amp:.1f} x over {int(same.sum())} samples, {amp_ev:.1f} x over the {int(ev.sum())} with early touchdowns; |X|max {scale:.1f}, "
              f"tolerance / 1e-12 = {sc.RTOL * scale / 1e-12:.0f}")
        assert ev.any() and amp * 1e-12 <= 0.01 * sc.RTOL * scale, (case, S, amp)


def test_two_pieces_on_the_host_hand_f_and_e_over(ter_emu, oracle_lib, solved_trot):
    """The program walked in two 24-step pieces with (F, E) handed over through its pointers equals the one 48-step run, bit for bit (a sample ends
    the first piece with E non-empty, asserted); a held sample writes neither back; and the reference started from that (F, E) agrees."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "block", xs)
    d1 = pkg.sim.Disturbance(seed=d.seed, u_max=d.u_max, kick_step=20)
    b, cut = 1, 23      # (the cut lies inside a phase: a swing foot that landed early is still a swing foot there)
    R = x0.shape[1]
    whole = tc.emu_run(ter_emu, pkg, so, b, x0[b], smap, 4, fz_rel, zg, ter, None, d1, k[b], MU)
    F, E = np.zeros((R, 4)), np.zeros((R, 4))
    first = tc.emu_run(ter_emu, pkg, so, b, x0[b], smap[:, :cut], 4, fz_rel, zg, ter, None, d1, k[b], MU, F=F, E=E)
    w = np.array([1, 2, 4, 8])
    live = first["rows"][:, 4] < 0
    assert np.array_equal((E * w).sum(axis=1), first["t"][:, 4]) and np.array_equal((F * w).sum(axis=1), first["c"][:, 4]) and (E[live].sum(axis=1) > 0).any()
    F2, E2 = F.copy(), E.copy()
    hold = np.zeros(R, dtype=np.int32); hold[3] = 1
    smap2 = np.ascontiguousarray(smap[:, cut:])
    d2 = pkg.sim.Disturbance(seed=d.seed, u_max=d.u_max)
    second = tc.emu_run(ter_emu, pkg, so, b, first["xf"], smap2, 4, fz_rel, zg, ter, None, d2, None, MU, F=F2, E=E2, hold=hold)
    assert np.array_equal(second["xf"][live], whole["xf"][live]) and np.array_equal(second["t"][live, 4], whole["t"][live, 4]) and np.array_equal(second["c"][live, 4], whole["c"][live, 4])
    assert np.array_equal(E2[3], E[3]) and np.array_equal(F2[3], F[3]) and np.array_equal((E2 * w).sum(axis=1)[hold == 0], second["t"][hold == 0, 4])
    rep = lambda a: a[None].repeat(b + 1, axis=0)
    ref = tc.oracle_walk_ter(pkg, oracle_lib, phases, pol, smap2, rep(first["xf"]), 4, fz_rel, zg, ter, d2, F0=rep(F > 0.5), E0=rep(E > 0.5))
    near = un.near_samples("host hand-over", {kk: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for kk, v in ref.items()})[0] | ~live
    got_c, got_t = un.contact_rows_of(pkg, second["c"]), tc.terrain_rows_of(pkg, second["t"])
    for f in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(got_c[f][~near], ref["rows"][f][b][~near]), f
    for f in tc.INTS_T:
        assert np.array_equal(got_t[f][~near], ref["trows"][f][b][~near]), f
    ok = ~near & (ref["first_bad"][b] < 0)
    sc.close("host hand-over x_final", second["xf"][ok], ref["X"][b, ok, -1])
    assert (ref["trows"]["n_held"][b][ok] > 0).any()      # the E of the first piece did act in the second


def test_host_build_refuses_what_the_library_refuses(ter_emu, solved_trot):
    """The refusals of hsddp_terrain_set that the host build shares: sizes, cell sizes, threshold, non-finite parameters, a map_of entry out of range."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 4)
    T = pkg.sim.Terrain
    H = np.zeros((2, 2, 2))
    bad = [T(H=H, cx=0.0), T(H=H, cy=-1.0), T(H=H, w_td=-1e-3), T(H=H, x0=np.nan), T(H=H, y0=np.inf), T(H=H, cx=np.inf), T(H=H, w_td=np.nan), T(H=np.zeros((1, 1, 1025))),
           T(H=np.zeros((1, 1025, 1))), T(H=np.zeros((4097, 1, 1))), T(H=np.zeros((1, 0, 1))), T(H=np.zeros((5, 1024, 1024)))]
    for t in bad:
        tc.emu_run(ter_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, t, expect=EINVAL)
    for mo in ([0, 0, 0, 0, 0, 0, 0, 2], [-1, 0, 0, 0, 0, 0, 0, 0]):
        tc.emu_run(ter_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, T(H=H), map_of=np.array(mo), expect=EINVAL)
    tc.emu_run(ter_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, T(H=H), map_of=np.array([0, 1] * 4))


def test_make_resources_ter():
    """Case 10: make resources-ter reports the three kernels at one wave per SIMD with at most 40 KiB of LDS.  Registers, spills and scratch are printed
    (DESIGN.md holds them beside their _uni twins), not asserted."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources-ter"], capture_output=True, text=True, check=True).stdout
    t, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            name = re.search(r"k_sim_quad[a-z0-9_]*ter", m.group(1)).group(0); t[name] = []
        else:
            t[name].append(m.group(1))
    assert sorted(t) == ["k_sim_quad_mc0_ter", "k_sim_quad_mc_ter", "k_sim_quad_ter"]
    for k, v in t.items():
        print("[ter]", k, "; ".join(v))
        assert "Occupancy [waves/SIMD]: 1" in v, k
        lds = [int(x.split(":")[1]) for x in v if x.startswith("LDS Size")]
        assert len(lds) == 1 and 0 < lds[0] <= 40 * 1024, (k, lds)


def test_walk_is_clean_under_the_sanitizers(tmp_path, solved_trot):
    """Case 11: tests/cpp/ter_walk_asan.cpp, a stand-alone program around the host build, compiled with -fsanitize=address,undefined and run on case 4
    and on base positions of 1e300 and NaN; it has to finish clean."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "edge", xs)
    b, S = 1, 5
    nph, hor, dt, al, ct, td, xb, ub, kk = tc.emu_args(pkg, so, b, x0[b], smap)
    parts = [[nph, 48, x0.shape[1], S, mc.PSI_DYN]]
    for p in range(nph):
        parts += [[hor[p], dt[p], al[p]], ct[p], td[p]]
    for p in range(nph):
        parts += [xb[p].ravel(), ub[p].ravel(), kk[p].ravel()]
    tp = ter.to_c()
    parts += [smap.ravel(), x0[b].ravel(), [d.kick_step], k[b].ravel(), [d.sigma_u, d.sigma_q, d.sigma_v, d.u_max, d.fall_height], [d.seed % (1 << 53)], [fz_rel, zg],
              [tp.nx, tp.ny, tp.n_maps, tp.early, tp.x0, tp.y0, tp.cx, tp.cy, tp.w_td], ter.grid().ravel(), np.zeros(x0.shape[1])]
    np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in parts]).tofile(str(tmp_path / "case.bin"))
    exe = str(tmp_path / "ter_walk_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ter_walk_asan.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path / "case.bin")], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "ter_walk_asan: clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_multiphase_ddp_header_compiles_with_terrain(tmp_path):
    """The C++ mirror: Simulation::set_terrain / terrain and Episode::set_terrain compile."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0, const double* H, const int* map_of) {\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8, true); std::vector<hsddp_terrain_row_t> rows(8);\n'
                   '    hsddp_terrain_t t = {2, 1, 1, 1, -9.85, 0.0, 10.0, 1.0, 0.05};\n'
                   '    bool ok = sim.set_contact(true, -10.0, 0.0) && sim.set_terrain(true, &t, H, map_of) && sim.run(x0) && sim.terrain(rows.data()) && sim.set_terrain(false);\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.set_contact(true, 0.0) && e.set_terrain(true, &t, H) && e.set_terrain(false); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
