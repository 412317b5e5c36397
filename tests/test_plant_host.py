"""CPU tests of the per-sample plant (include/hsddp_plant.h): the ctypes mirror, payload_trunk against a brute-force sum of point masses, the restated
reference walks of tests/plant_common.py against the originals at a nominal table, the ten programs (cafe-mpc_amd/csrc/wb_sim.hpp with the PLANT
policies) compiled for the host by tests/_emu/plant_emu.cpp against those references, isolation of the samples, the refusals the host validation shares
with the library, make resources-plant, a sanitizer run of a stand-alone program around the validation and the packing, and the C++ mirror.  The
library's own refusals, toggling and episodes need the library: tests/test_plant_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import sim_common as sc
import mc_common as mc
import sub_common as sub
import uni_common as un
import ter_common as tc
import plant_common as pc

MU = 0.6
EINVAL = -1
Plant = pkg.sim.Plant


def test_plant_abi_mirror_matches_the_header():
    """Every prototype of include/hsddp_plant.h is in PLANT_EXPORTS and in no other list; bind_plant refuses a library that lacks one; the constants are
    the header's; the earlier binders still bind a library without the new symbols."""
    src = open(os.path.join(ROOT, "include", "hsddp_plant.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = set(re.findall(r"\b(hsddp_plant_[a-z_]+)\s*\(", code))
    A = pkg._abi
    assert protos == set(A.PLANT_EXPORTS) and len(protos) == 3
    others = (set(A.EXPORTS) | set(A.ENSEMBLE_EXPORTS) | set(A.HKD_EXPORTS) | set(A.REFS_EXPORTS) | set(A.SIM_EXPORTS) | set(A.MC_EXPORTS) | set(A.GRF_EXPORTS)
              | set(A.EPISODE_EXPORTS) | set(A.SUBSTEP_EXPORTS) | set(A.CONTACT_EXPORTS) | set(A.TERRAIN_EXPORTS))
    assert not protos & others
    assert (len(A.SIM_EXPORTS), len(A.MC_EXPORTS), len(A.GRF_EXPORTS), len(A.EPISODE_EXPORTS), len(A.SUBSTEP_EXPORTS), len(A.CONTACT_EXPORTS), len(A.TERRAIN_EXPORTS)) == (7, 2, 2, 9, 2, 3, 3)
    assert int(re.search(r"#define HSDDP_PLANT_ROW (\d+)", code).group(1)) == A.PLANT_ROW == 46 and int(re.search(r"#define HSDDP_PLANT_MAX (\d+)", code).group(1)) == A.PLANT_MAX
    assert len(A.PLANT_NOMINAL) == A.PLANT_ROW and sorted((s.start, s.stop) for s in A.PLANT_SLICES.values()) == [(0, 1), (1, 4), (4, 10), (10, 22), (22, 34), (34, 46)]
    nom = np.array(A.PLANT_NOMINAL)
    assert nom[0] == 3.3 and not nom[1:4].any() and list(nom[4:10]) == [0.011253, 0, 0, 0.036203, 0, 0.042673] and (nom[10:34] == 1).all() and not nom[34:].any()

    class Fake:
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.CONTACT_EXPORTS + A.TERRAIN_EXPORTS:
        setattr(lib, s, Fake())
    A.bind_terrain(lib); A.bind_contact(lib)      # a library without the new symbols
    for s in A.PLANT_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_plant(lib)
    setattr(lib, A.PLANT_EXPORTS[-1], Fake())
    A.bind_plant(lib)
    assert len(lib.hsddp_plant_set.argtypes) == 5 and len(lib.hsddp_plant_get_params.argtypes) == 3 and len(lib.hsddp_plant_get_table.argtypes) == 4


def test_payload_trunk_is_the_sum_of_point_masses():
    """payload_trunk against a brute-force model: the nominal trunk as eight point masses at the corners of its equivalent box (same mass, CoM and
    inertia) plus a payload of point masses; total mass, first moment and inertia about the ORIGIN of the union, to rounding."""
    nom = np.array(pkg._abi.PLANT_NOMINAL)
    m0, (Ixx, Iyy, Izz) = nom[0], nom[[4, 7, 9]]
    half = np.sqrt(np.array([Iyy + Izz - Ixx, Ixx + Izz - Iyy, Ixx + Iyy - Izz]) / (2.0 * m0))      # eight masses m0 / 8 at (+-a, +-b, +-c): Ixx = m0 (b^2 + c^2)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    pts = [(m0 / 8.0, c) for c in corners]
    about0 = lambda pts: sum(m * (float(p @ p) * np.eye(3) - np.outer(p, p)) for m, p in pts)
    assert np.allclose(about0(pts), np.diag([Ixx, Iyy, Izz]), rtol=1e-13, atol=0)
    pos = np.array([0.08, 0.03, 0.05])
    pay = [(0.5, pos + np.array([0.02, 0.01, -0.015])), (0.5, pos - np.array([0.02, 0.01, -0.015])), (0.5, pos + np.array([-0.01, 0.03, 0.0])), (0.5, pos - np.array([-0.01, 0.03, 0.0]))]
    mp = sum(m for m, _ in pay)
    Ip = sum(m * (float((p - pos) @ (p - pos)) * np.eye(3) - np.outer(p - pos, p - pos)) for m, p in pay)      # the payload about its own centre
    six = lambda M: np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])
    for inertia, union in ((None, pts + [(mp, pos)]), (six(Ip), pts + pay)):
        m, c, I = pkg.sim.payload_trunk(mp, pos, inertia)
        mass = sum(w for w, _ in union); first = sum(w * p for w, p in union)
        assert abs(m - mass) <= 1e-15 * mass and np.allclose(m * c, first, rtol=1e-14, atol=1e-18)
        Ic = np.array([[I[0], I[1], I[2]], [I[1], I[3], I[4]], [I[2], I[4], I[5]]])
        I0 = Ic + m * (float(c @ c) * np.eye(3) - np.outer(c, c))
        assert np.allclose(I0, about0(union), rtol=1e-13, atol=1e-18)
    assert pkg.sim.payload_trunk(0.0, (0.3, 0.2, 0.1))[0] == 3.3 and np.array_equal(pkg.sim.payload_trunk(0.0, (0.3, 0.2, 0.1))[2], nom[4:10])
    row = pkg.sim.with_damping(pkg.sim.with_gain(pkg.sim.with_link_scale(nom, (0.8, 1.2, 1.1)), 0.9), np.arange(12) * 0.001)
    assert list(row[10:16]) == [0.8, 1.2, 1.1, 0.8, 1.2, 1.1] and (row[22:34] == 0.9).all() and np.array_equal(row[34:], np.arange(12) * 0.001) and np.array_equal(row[:10], nom[:10])
    with pytest.raises(ValueError):
        pkg.sim.with_gain(nom, np.ones(5))
    assert Plant.nominal(3).table().shape == (3, 46) and Plant(nom).table().shape == (1, 46)
    with pytest.raises(ValueError):
        Plant(np.zeros((2, 45))).table()


@pytest.fixture(scope="module")
def plant_emu(tmp_path_factory):
    return pc.build_emu(tmp_path_factory.mktemp("plant_emu"))


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return pc.build_ref(pkg, tmp_path_factory.mktemp("plant_ref"))


@pytest.fixture(scope="module")
def solved_trot(oracle_lib):
    """The fixture of tests/test_terrain_host.py: trot 4 x 12, four problems, 3 AL x 4 DDP iterations, eight samples around Xbar[0] (sigma 0.02 / 0.2)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, so, xs, mc.policy_of(so)
    so.close()


def test_restated_walks_are_the_originals_at_nominal(ref_lib, oracle_lib, solved_trot):
    """With a nominal table every array the restated walks return equals the original walk's, bit for bit - and a non-nominal row changes it, and the
    walk after it is the original again (the links are restored)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    D = mc.cases(pkg, (2, 3))["D"]
    for S, d, k in ((2, None, None), (3, D[0], D[1])):
        a = pc.oracle_walk_sub_plant(pkg, ref_lib, phases, pol, smap, xs[:2, :3], S, Plant.nominal(), d, k)
        b = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs[:2, :3], S, d, k)
        assert set(a) == set(b)
        for f in b:
            assert np.array_equal(a[f], b[f]), (S, f)
    x0, d, k, fz_rel, zg, ter = tc.case_setup(pkg, "block", xs)
    args = (phases, pol, smap, x0[:2, 5:], 4, fz_rel, zg)
    b = tc.oracle_walk_ter(pkg, oracle_lib, *args, ter, d, k[:2, 5:])
    moved = pc.oracle_walk_ter_plant(pkg, ref_lib, *args, ter, pc.mixed_table(pkg, (2, 3)), d, k[:2, 5:])
    a = pc.oracle_walk_ter_plant(pkg, ref_lib, *args, ter, Plant.nominal(), d, k[:2, 5:])
    assert set(a) == set(b) and b["trows"]["n_early"].sum() > 0 and b["rows"]["n_release"].sum() > 0
    for f in b:
        same = (a[f] == b[f]) if isinstance(b[f], (set, tuple)) else (a[f].tobytes() == b[f].tobytes())
        assert same, f
    assert np.abs(moved["X"][0, 1] - b["X"][0, 1]).max() > 1e-3 and np.array_equal(moved["X"][0, 0], b["X"][0, 0])
    x0, d, k, fz_rel, zg = un.case_setup(pkg, "flight", xs)      # the contact rule alone: the flat one-cell map
    a = pc.oracle_walk_ter_plant(pkg, ref_lib, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, None, Plant.nominal(), d, k[:2, 5:])
    b = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, d, k[:2, 5:])
    for f in ("X", "U", "Y", "att", "F", "solves", "force_margin", "kin_margin"):
        assert np.array_equal(a[f], b[f]), f
    assert a["rows"].tobytes() == b["rows"].tobytes() and b["rows"]["n_release"].sum() > 0


@pytest.mark.parametrize("family,case,S,table", pc.CASES)
def test_programs_on_the_host_match_the_reference(plant_emu, ref_lib, solved_trot, family, case, S, table):
    """The host build of the walks with a mixed three-row table against the restated reference walks.  Non-vacuity first, on the references alone: every
    sample of a non-nominal row moves by more than 1e-3 in X against the walk at nominal (measured: 0.43 .. 1.8 on the plain cases, 2.9 .. 8.7 under
    case D with gains and friction, up to 170 where a kicked sample lands differently); and the cap of one left-out sample (measured: plain S = 1 and
    S = 3 leave out one sample each at 0.82 / 0.95 of the record margin, the block one at a record threshold, the others none)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, pl = pc.case_of(pkg, family, case, S, table, xs)
    ref = pc.reference_of(pkg, ref_lib, phases, pol, smap, family, x0, S, fz_rel, zg, ter, pl, d, k)
    nominal = pc.reference_of(pkg, ref_lib, phases, pol, smap, family, x0, S, fz_rel, zg, ter, Plant.nominal(), d, k)
    live = (ref["first_bad"] < 0) & (nominal["first_bad"] < 0)
    pc.assert_table_moves_the_reference(f"host {case} S={S}", {"X": ref["X"][live][None]}, {"X": nominal["X"][live][None]}, Plant(pl.rows, plant_of=np.asarray(pl.plant_of)[live][None]))
    res = pc.host_run(plant_emu, pkg, so, x0, smap, S, pl, family, fz_rel, zg, ter, d, k, MU)
    contact = np.array([[phases[int(p)]["desc"].contact[l] for l in range(4)] for p in smap[0]])
    pc.compare(pkg, f"host {case} S={S}", family, res, ref, mc.xbar_window(pol, smap)[:x0.shape[0]], contact, MU, fz_rel)
    if case == "divergence":
        assert ref["first_bad"][1, 1] == 5 and res["rows"]["first_bad"][1, 1] == 5


@pytest.fixture(scope="module")
def ter_emu(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("ter_emu_for_plant"))


def test_samples_are_isolated_on_the_host(plant_emu, ter_emu, solved_trot):
    """The samples of a nominal row are bit-identical to a run with a one-row nominal table; permuting the rows of the table and re-indexing plant_of
    changes no bit; and a nominal table gives the integers of the program without the plant and its floats within the tolerance (every added operation
    is exact at nominal - x 1, + 0, - 0 qdot - so bit-identity is expected: printed)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, pl = pc.case_of(pkg, "ter", "block", 4, "mixed2", xs)
    res = pc.host_run(plant_emu, pkg, so, x0, smap, 4, pl, "ter", fz_rel, zg, ter, d, k, MU)
    alone = pc.host_run(plant_emu, pkg, so, x0, smap, 4, Plant.nominal(), "ter", fz_rel, zg, ter, d, k, MU)
    n0 = np.asarray(pl.plant_of) == 0
    for f in res:
        assert res[f][n0].tobytes() == alone[f][n0].tobytes(), f
    assert not np.array_equal(res["x_final"][~n0], alone["x_final"][~n0])
    perm = np.array([2, 0, 1])      # new row i is old row perm[i]
    inv = np.argsort(perm)
    shuffled = pc.host_run(plant_emu, pkg, so, x0, smap, 4, Plant(pl.rows[perm], plant_of=inv[np.asarray(pl.plant_of)].astype(np.int32)), "ter", fz_rel, zg, ter, d, k, MU)
    for f in res:
        assert res[f].tobytes() == shuffled[f].tobytes(), f
    base = tc.host_run(ter_emu, pkg, so, x0, smap, 4, fz_rel, zg, ter, d, k, MU)
    print(f"[plant] host block, nominal table: bit-identical to the program without the plant: {all(alone[f].tobytes() == base[f].tobytes() for f in base)}")
    for f in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(alone["contact"][f], base["contact"][f]), f
    for f in tc.INTS_T:
        assert np.array_equal(alone["terrain"][f], base["terrain"][f]), f
    assert np.array_equal(alone["rows"]["first_bad"], base["rows"]["first_bad"]) and np.array_equal(alone["grf"]["n_slip"], base["grf"]["n_slip"]) and np.array_equal(alone["extra"], base["extra"])
    for f in ("X", "U", "x_final", "Y"):
        sc.close(f"host nominal {f}", alone[f], base[f], scale=max(1.0, float(np.abs(base[f]).max())))


def test_pending_impact_on_the_host_uses_the_robot_s_links(plant_emu, ref_lib, solved_trot):
    """The episode's pending reset map (wbs_plant_impact, the program of k_episode_impact_plant) on four robots with the three rows against the oracle's
    impact with those links; a frozen robot is left alone; the heavier robots' velocities differ from the nominal one's."""
    phases, so, xs, pol = solved_trot
    D = [p["desc"] for p in phases]
    pi = next(i for i, q in enumerate(D) if any(q.contact[l] == 0 and q.next_contact[l] == 1 for l in range(4)))
    hor = np.array([q.horizon for q in D], dtype=np.int32); dt = np.array([q.dt for q in D]); al = np.array([q.BG_alpha for q in D])
    ct = np.array([[q.contact[l] for l in range(4)] for q in D], dtype=np.int32)
    td = np.array([[1 if (q.contact[l] == 0 and q.next_contact[l] == 1) else 0 for l in range(4)] for q in D], dtype=np.int32)
    state = np.ascontiguousarray(xs[:, 3]).copy(); before = state.copy(); x0 = np.full((4, 36), np.nan)
    rows = pc.three_rows(pkg); po = np.array([1, 0, 2, 2], dtype=np.int32); frozen = np.array([0, 0, 0, 1], dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = plant_emu.plant_emu_impact(len(D), vp(hor), vp(dt), vp(al), vp(ct), vp(td), ctypes.c_double(mc.PSI_DYN), pi, 4, vp(frozen), vp(state), vp(x0), 3, vp(rows), vp(po))
    assert rc == 0
    for b in range(3):
        want = pc.impact_ref(pkg, ref_lib, D[pi], before[b], rows[po[b]])
        sc.close(f"impact robot {b}", state[b], want); assert np.array_equal(x0[b], state[b]) and np.array_equal(state[b, :18], before[b, :18])
    assert np.array_equal(state[3], before[3]) and np.isnan(x0[3]).all()
    nominal = pc.impact_ref(pkg, ref_lib, D[pi], before[0], rows[0])
    assert np.abs(state[0] - nominal).max() > 1e-3
    assert plant_emu.plant_emu_impact(len(D), vp(hor), vp(dt), vp(al), vp(ct), vp(td), ctypes.c_double(mc.PSI_DYN), pi, 4, vp(frozen), vp(state), vp(x0), 3, vp(rows), vp(np.array([0, 1, 2, 3], dtype=np.int32))) == EINVAL


def test_host_validation_refuses_what_the_library_refuses(plant_emu, solved_trot):
    """Every refusal of the header that concerns the table, on the validation the library, the host build and the sanitizer program share; and through
    the host build's run."""
    phases, so, xs, pol = solved_trot
    P, po, bad = pc.bad_tables(pkg)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    ok = lambda n, rows, of: plant_emu.plant_emu_table_ok(n, vp(rows), vp(of), ctypes.c_longlong(8))
    assert ok(3, P, po) == 1 and ok(3, P, None) == 1 and ok(1, P, None) == 1
    assert ok(0, P, po) == 0 and ok(-1, P, po) == 0 and ok(65537, P, None) == 0 and ok(2, P, po) == 0
    for rows, of in bad:
        assert ok(3, rows, of) == 0
    assert ok(3, np.where(np.arange(46) == 25, -1.0, P), po) == 1      # any finite gain is a plant
    smap = sc.step_map(phases, 4)
    for rows, of in bad[1:4] + bad[-2:]:
        pc.emu_run(plant_emu, pkg, so, 0, xs[0], smap, 2, rows, of, expect=EINVAL)
    pc.emu_run(plant_emu, pkg, so, 0, xs[0], smap, 2, None, po, expect=EINVAL)
    pc.emu_run(plant_emu, pkg, so, 0, xs[0], smap, 2, P, po)


def test_make_resources_plant():
    """make resources-plant lists exactly the ten kernels, each at one wave per SIMD with at most 40 KiB of LDS.  Registers, spills and scratch are
    printed (DESIGN.md holds them), not asserted.  (That make resources is unchanged for every existing kernel is held by
    tests/test_contact_host.py::test_make_resources_leaves_every_existing_kernel_alone.)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources-plant"], capture_output=True, text=True, check=True).stdout
    t, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            name = re.search(r"k_(sim_quad|episode_impact)[a-z0-9_]*plant", m.group(1)).group(0); t[name] = []
        else:
            t[name].append(m.group(1))
    assert sorted(t) == sorted(["k_sim_quad_plant", "k_sim_quad_mc_plant", "k_sim_quad_mc0_plant", "k_sim_quad_uni_plant", "k_sim_quad_mc_uni_plant", "k_sim_quad_mc0_uni_plant",
                                "k_sim_quad_ter_plant", "k_sim_quad_mc_ter_plant", "k_sim_quad_mc0_ter_plant", "k_episode_impact_plant"])
    for k, v in t.items():
        print("[plant]", k, "; ".join(v))
        assert "Occupancy [waves/SIMD]: 1" in v, k
        lds = [int(x.split(":")[1]) for x in v if x.startswith("LDS Size")]
        assert len(lds) == 1 and 0 <= lds[0] <= 40 * 1024 and (lds[0] > 0 or k == "k_episode_impact_plant"), (k, lds)


def test_table_code_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/plant_table_asan.cpp, a stand-alone program around the host-side validation and packing (cafe-mpc_amd/csrc/plant_host.hpp), compiled
    with -fsanitize=address,undefined and run directly; it has to finish clean."""
    exe = str(tmp_path / "plant_table_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "plant_table_asan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "plant_table_asan: clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_multiphase_ddp_header_compiles_with_plant(tmp_path):
    """The C++ mirror: Simulation::set_plant / plant and Episode::set_plant compile."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0, const double* P, const int* plant_of) {\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8, true); bool on = false;\n'
                   '    bool ok = sim.set_plant(true, 3, P, plant_of) && sim.run(x0) && sim.plant(&on).size() == 3 * HSDDP_PLANT_ROW && sim.set_plant(false);\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.set_plant(true, 3, P) && e.set_plant(false); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
