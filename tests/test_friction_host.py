"""CPU tests of Coulomb friction (include/hsddp_friction.h): the ctypes mirror, the reference walk of tests/fric_common.py against the terrain reference at
mu_s = 1e9, and the program itself (cafe-mpc_amd/csrc/wb_sim.hpp with the FRIC policies) compiled for the host by tests/_emu/fric_emu.cpp against that
reference - without an event, under a lateral push at S = 1 and 4, on a partial wave, under noise, on the block terrain, on a contained divergence, and in
two pieces with (F, E, Sl, n_f) handed over.  Plus the records' rule, the amplification through the windows, the pick rule, make resources-fric and the
C++ mirror.  Toggling, the library's refusals and episodes need the library: tests/test_friction_gpu.py."""
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
import fric_common as fc

MU = 0.6
EINVAL = -1


def test_friction_abi_mirror_matches_the_header():
    """Every prototype of include/hsddp_friction.h is in FRICTION_EXPORTS and in no other list; bind_friction refuses a library that lacks one; the row
    dtype and the parameter structure have the layouts of hsddp_friction_row_t and hsddp_friction_t."""
    src = open(os.path.join(ROOT, "include", "hsddp_friction.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = set(re.findall(r"\b(hsddp_friction_[a-z_]+)\s*\(", code))
    A = pkg._abi
    assert protos == set(A.FRICTION_EXPORTS) and len(protos) == 3
    others = (set(A.EXPORTS) | set(A.ENSEMBLE_EXPORTS) | set(A.HKD_EXPORTS) | set(A.REFS_EXPORTS) | set(A.SIM_EXPORTS) | set(A.MC_EXPORTS) | set(A.GRF_EXPORTS)
              | set(A.EPISODE_EXPORTS) | set(A.SUBSTEP_EXPORTS) | set(A.CONTACT_EXPORTS) | set(A.TERRAIN_EXPORTS) | set(A.PLANT_EXPORTS))
    assert not protos & others

    def members(struct):
        body = re.search(r"typedef struct \{([^{}]*)\} " + struct + ";", code).group(1)
        return [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert members("hsddp_friction_row_t") == list(A.FRICTION_ROW_DTYPE.names) and A.FRICTION_ROW_DTYPE.itemsize == 40 and A.FRICTION_ROW_DTYPE.fields["max_speed"][1] == 24
    assert members("hsddp_friction_t") == [f for f, _ in A.FrictionParams._fields_] and ctypes.sizeof(A.FrictionParams) == 16 and A.FrictionParams.n_mu.offset == 8

    class Fake:
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.CONTACT_EXPORTS + A.TERRAIN_EXPORTS + A.FRICTION_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_friction(lib)
    setattr(lib, A.FRICTION_EXPORTS[-1], Fake())
    A.bind_friction(lib)
    assert len(lib.hsddp_friction_set.argtypes) == 5 and len(lib.hsddp_friction_get_params.argtypes) == 3
    t = pkg.sim.Friction(0.6).table()
    assert t.shape == (1, 2) and (t == 0.6).all() and pkg.sim.Friction((0.7, 0.5)).table().tolist() == [[0.7, 0.5]]


@pytest.fixture(scope="module")
def fric_emu(tmp_path_factory):
    return fc.build_emu(tmp_path_factory.mktemp("fric_emu"))


@pytest.fixture(scope="module")
def fric_ref(tmp_path_factory):
    return fc.build_ref(pkg, tmp_path_factory.mktemp("fric_ref"))


@pytest.fixture(scope="module")
def ter_emu(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("ter_emu_for_fric"))


@pytest.fixture(scope="module")
def uni_emu(tmp_path_factory):
    return un.build_emu(tmp_path_factory.mktemp("uni_emu_for_fric"))


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


def reference(refs, fric_ref, solved_trot, case, S):
    phases, so, xs, pol = solved_trot
    if (case, S) not in refs:
        x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, case, xs)
        refs[(case, S)] = fc.oracle_walk_fric(pkg, fric_ref, phases, pol, sc.step_map(phases, 48), x0, S, fz_rel, zg, ter, fr, d, k)
    return refs[(case, S)]


def test_reference_walk_at_mu_1e9_is_the_terrain_reference(oracle_lib, fric_ref, solved_trot):
    """The reference itself: at mu_s = 1e9 (no foot ever leaves the cone) it is ter_common.oracle_walk_ter on the flat map, bit for bit - through
    fric_ref_dynamics, which without a sliding foot is the oracle's own solve statement for statement."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, "none", xs)
    flat = tc.terrain_of(pkg, "flat", x0.shape[:2])
    a = fc.oracle_walk_fric(pkg, fric_ref, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, None, fr, d, k[:2, 5:])
    b = tc.oracle_walk_ter(pkg, oracle_lib, phases, pol, smap, x0[:2, 5:], 2, fz_rel, zg, flat, d, k[:2, 5:])
    for f in ("X", "U", "Y", "att", "F", "E", "solves", "kin_margin"):
        assert np.array_equal(a[f], b[f]), f
    assert a["rows"].tobytes() == b["rows"].tobytes() and a["trows"].tobytes() == b["trows"].tobytes() and b["rows"]["n_release"].sum() > 0
    f = a["frows"]
    assert (f["first_slide"] == -1).all() and not any(f[n].any() for n in ("n_onset", "n_slide", "n_restick", "slide_final", "max_speed", "distance"))
    assert not a["slide"].any()


def test_no_event_on_the_host_is_the_program_without_friction(fric_emu, ter_emu, uni_emu, solved_trot):
    """Case 1: mu_s = 1e9, S = 3, 4 x 8 samples: bit-identical to the program with the terrain (flat map) AND to the one with the contact rule alone; the
    friction rows are all zero / -1.  The case runs at fz_rel = 0, not the fixture's -10 N: a foot that pulls (fz_rel < lambda_z < 0) is outside the cone
    at any mu, so at -10 N the rule has eleven onsets even at mu_s = 1e9 (fric_common SIZING, and the header's note on pulling feet)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, "none", xs)
    res = fc.host_run(fric_emu, pkg, so, x0, smap, 3, fz_rel, zg, None, fr, d, k, MU)
    with_ter = tc.host_run(ter_emu, pkg, so, x0, smap, 3, fz_rel, zg, tc.terrain_of(pkg, "flat", x0.shape[:2]), d, k, MU)
    base = un.host_run(uni_emu, pkg, so, x0, smap, 3, fz_rel, zg, d, k, MU)
    f = res.pop("friction"); with_ter.pop("terrain")
    assert base["contact"]["n_release"].sum() > 0 and base["contact"]["n_land"].sum() > 0
    for name in base:
        assert res[name].tobytes() == with_ter[name].tobytes(), name
    for name in base:      # (tests/test_terrain_host.py prints, and does not assert, this identity for the _ter program on its own input; here it is held)
        assert res[name].tobytes() == base[name].tobytes(), name
    for n in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(res["contact"][n], base["contact"][n]), n
    assert (f["first_slide"] == -1).all() and not any(f[n].any() for n in ("n_onset", "n_slide", "n_restick", "slide_final", "max_speed", "distance"))


@pytest.mark.parametrize("case,S", fc.CASES)
def test_program_on_the_host_matches_the_reference(fric_emu, fric_ref, solved_trot, refs, case, S):
    """Cases 2 - 6 of fric_common.case_setup against the reference walk; the non-vacuity of each case is asserted on the REFERENCE, and so is the cap of one
    left-out sample, before anything is compared."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, case, xs)
    ref = reference(refs, fric_ref, solved_trot, case, S)
    fc.assert_case_is_not_vacuous(case, ref, S)
    res = fc.host_run(fric_emu, pkg, so, x0, smap, S, fz_rel, zg, ter, fr, d, k, MU)
    fc.compare_case(f"host {case} S={S}", pkg, res, ref, mc.xbar_window(pol, smap)[:x0.shape[0]], MU, 0.0, fz_rel)
    if case == "divergence":      # the sample that fails the test in a sliding substep keeps the state and the counters of that moment
        assert res["rows"]["first_bad"][1, 1] == 5 and np.array_equal(res["X"][1, 1, 6:], np.broadcast_to(res["x_final"][1, 1], (43, 36)))
        assert res["friction"]["n_slide"][1, 1] == ref["frows"]["n_slide"][1, 1] > 0


def test_records_hold_the_cone_over_the_sticking_feet(fric_emu, fric_ref, solved_trot, refs):
    """Case 7: with the records' mu equal to mu_s, min_cone >= 0 on every sample (up to the force bound) and n_slip counts normal-force violations alone;
    Y of a sliding foot is (f_t, lambda_z) with |f_t| = mu_k n_f of the substep, which is at most mu_k times the largest normal force of the run."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, _ = fc.case_setup(pkg, "push", xs)
    fr = pkg.sim.Friction(mu=[[fc.MU_LOW, fc.MU_LOW_K]], v_stick=fc.V_STICK)
    res = fc.host_run(fric_emu, pkg, so, x0, smap, 4, fz_rel, zg, None, fr, d, k, fc.MU_LOW)
    ref = fc.oracle_walk_fric(pkg, fric_ref, phases, pol, smap, x0, 4, fz_rel, zg, None, fr, d, k)
    fb = gc.force_bound(ref["Y"])
    assert ref["frows"]["n_onset"].sum() > 0 and res["friction"]["n_slide"].sum() > 0
    fin = np.isfinite(res["grf"]["min_cone"])
    assert fin.all() and (res["grf"]["min_cone"] >= -fb).all(), res["grf"]["min_cone"].min()
    sl0 = ref["slide"][..., 0, :]      # Y holds the first substep of a control step
    Yf = res["Y"].reshape(res["Y"].shape[:-1] + (4, 3))
    keep = ~un.near_samples("host records", ref)
    assert sl0[keep].any()
    ft = np.hypot(Yf[..., 0], Yf[..., 1])
    assert (ft[keep][sl0[keep]] <= fc.MU_LOW_K * res["grf"]["max_fz"].max() + fb).all()
    # the same run under glue leaves the pyramid: that is what the rule removes
    glue = fc.host_run(fric_emu, pkg, so, x0, smap, 4, fz_rel, zg, None, pkg.sim.Friction(mu=[[fc.MU_BIG, fc.MU_BIG]]), d, k, fc.MU_LOW)
    assert (glue["grf"]["min_cone"] < -1.0).any()


def test_amplification_through_the_friction_windows(fric_emu, solved_trot):
    """A 1e-12 change of x0 through the 48-step windows of the cases on the host build, over the samples that keep their decisions: printed, and at least
    two orders below the tolerance the windows are held to, 1e-8 x max(1, |X|max) (sim_common.close)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    rng = np.random.default_rng(7)
    for case, S in fc.CASES[:5]:
        x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, case, xs)
        a = fc.host_run(fric_emu, pkg, so, x0, smap, S, fz_rel, zg, ter, fr, d, k, MU)
        b = fc.host_run(fric_emu, pkg, so, x0 + 1e-12 * rng.uniform(-1.0, 1.0, x0.shape), smap, S, fz_rel, zg, ter, fr, d, k, MU)
        same = np.all([a["contact"][f] == b["contact"][f] for f in fc.INTS_C] + [a["friction"][f] == b["friction"][f] for f in fc.INTS_F], axis=0) & (a["rows"]["first_bad"] < 0)
        ev = same & (a["friction"]["n_onset"] > 0)
        amp = np.abs(a["X"][same] - b["X"][same]).max() / 1e-12
        amp_ev = np.abs(a["X"][ev] - b["X"][ev]).max() / 1e-12 if ev.any() else 0.0
        scale = max(1.0, float(np.abs(a["X"][same]).max()))
        print(f"[fric] amplification {case} S={S}: {amp:.1f} x over {int(same.sum())} of {same.size} samples, {amp_ev:.1f} x over the {int(ev.sum())} that slide; |X|max {scale:.1f}, "
              f"tolerance / 1e-12 = {sc.RTOL * scale / 1e-12:.0f}")
        assert ev.any() and same.sum() >= same.size - 3 and amp * 1e-12 <= 0.01 * sc.RTOL * scale, (case, S, amp)


def test_two_pieces_on_the_host_hand_the_sliding_set_over(fric_emu, fric_ref, solved_trot):
    """The program walked in two pieces with (F, E, Sl, n_f) handed over through its pointers equals the one 48-step run, bit for bit (a sample ends the
    first piece with Sl non-empty, asserted); a held sample writes nothing back; and the reference started from that state agrees."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg, ter, fr = fc.case_setup(pkg, "push", xs)
    b, R = 3, x0.shape[1]
    fo = np.asarray(fr.mu_of)[b]
    d0 = pkg.sim.Disturbance(seed=d.seed, u_max=d.u_max)
    whole = fc.emu_run(fric_emu, pkg, so, b, x0[b], smap, 4, fz_rel, zg, None, fr, fo, None, d0, None, MU)
    live = whole["rows"][:, 4] < 0
    w = np.array([1, 2, 4, 8])
    cut = None
    for c in range(14, 46):      # a cut inside a phase at which a sample is sliding
        F, E, Sl, NF = (np.zeros((R, 4)) for _ in range(4))
        first = fc.emu_run(fric_emu, pkg, so, b, x0[b], smap[:, :c], 4, fz_rel, zg, None, fr, fo, None, d0, None, MU, F=F, E=E, Sl=Sl, NF=NF)
        if (Sl[live].sum(axis=1) > 0).any() and smap[1, c] != 0:
            cut = c
            break
    assert cut is not None, "no cut with a sliding foot"
    assert np.array_equal((Sl * w).sum(axis=1), first["f"][:, 4]) and (NF[Sl > 0.5] >= 0.0).all()
    F2, E2, Sl2, NF2 = F.copy(), E.copy(), Sl.copy(), NF.copy()
    hold = np.zeros(R, dtype=np.int32); hold[3] = 1
    smap2 = np.ascontiguousarray(smap[:, cut:])
    second = fc.emu_run(fric_emu, pkg, so, b, first["xf"], smap2, 4, fz_rel, zg, None, fr, fo, None, d0, None, MU, F=F2, E=E2, Sl=Sl2, NF=NF2, hold=hold)
    assert np.array_equal(second["xf"][live], whole["xf"][live]) and np.array_equal(second["f"][live, 4], whole["f"][live, 4])
    assert np.array_equal(first["f"][live, 1:4] + second["f"][live, 1:4], whole["f"][live, 1:4])      # onsets, sliding pairs and re-sticks add up
    assert np.array_equal(Sl2[3], Sl[3]) and np.array_equal(NF2[3], NF[3]) and np.array_equal((Sl2 * w).sum(axis=1)[hold == 0], second["f"][hold == 0, 4])
    rep = lambda a: a[None].repeat(b + 1, axis=0)
    fr2 = pkg.sim.Friction(mu=fr.mu, mu_of=rep(fo), v_stick=fr.v_stick)
    ref = fc.oracle_walk_fric(pkg, fric_ref, phases, pol, smap2, rep(first["xf"]), 4, fz_rel, zg, None, fr2, d0, F0=rep(F > 0.5), E0=rep(E > 0.5), Sl0=rep(Sl > 0.5), NF0=rep(NF))
    near = un.near_samples("host hand-over", {kk: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for kk, v in ref.items()})[0] | ~live
    got = fc.friction_rows_of(pkg, second["f"])
    for f in fc.INTS_F:
        assert np.array_equal(got[f][~near], ref["frows"][f][b][~near]), f
    ok = ~near & (ref["first_bad"][b] < 0)
    sc.close("host hand-over x_final", second["xf"][ok], ref["X"][b, ok, -1], scale=max(1.0, float(np.abs(ref["X"][b, ok]).max())))


def test_host_build_refuses_what_the_library_refuses(fric_emu, solved_trot):
    """The refusals of hsddp_friction_set that the host build shares: an empty table, non-finite or negative values, mu_k > mu_s, an index out of range."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 4)
    Fr = pkg.sim.Friction
    for fr in (Fr(mu=[[0.5, 0.6]]), Fr(mu=[[-0.1, -0.2]]), Fr(mu=[[0.5, -0.1]]), Fr(mu=[[np.nan, 0.1]]), Fr(mu=[[np.inf, np.inf]]), Fr(mu=[[0.5, 0.4]], v_stick=-1e-3),
               Fr(mu=[[0.5, 0.4]], v_stick=np.nan), Fr(mu=np.zeros((0, 2)))):
        fc.emu_run(fric_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, None, fr, expect=EINVAL)
    for mo in ([0, 0, 0, 0, 0, 0, 0, 2], [-1, 0, 0, 0, 0, 0, 0, 0]):
        fc.emu_run(fric_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, None, Fr(mu=[[0.5, 0.4], [0.3, 0.0]]), mu_of=np.array(mo), expect=EINVAL)
    fc.emu_run(fric_emu, pkg, so, 0, xs[0], smap, 1, -10.0, 0.0, None, Fr(mu=[[0.5, 0.4], [0.3, 0.0]]), mu_of=np.array([0, 1] * 4))


def test_pick_rule_with_friction(tmp_path):
    """Case 10: tests/cpp/sim_pick_fric_table.cpp walks all 256 settings of the rule under the sanitizers - 30 kernels reachable, friction without the
    contact rule inert, the plant combination flagged - and tests/cpp/sim_pick_table.cpp, unchanged, still answers clean: with the switch off the 27
    kernels are what is reachable."""
    for name, word in (("sim_pick_fric_table", "sim_pick_fric_table: clean"), ("sim_pick_table", "sim_pick_table: clean")):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "cafe-mpc_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        print(r.stdout + r.stderr)
        assert r.returncode == 0 and word in r.stdout and "runtime error" not in r.stderr


def test_friction_kernels_live_in_a_library_of_their_own(tmp_path):
    """The product build links hsddp_fric.o into libhsddp_fric.so: its gfx950 code object defines exactly the three friction walks, libhsddp_hip.so needs
    it and looks for it beside itself, and defines none of them - its fat binary holds the code objects it held before friction existed.  The one-command
    build takes the file in through hsddp_hip.hip (its kernels against the product's: tests/test_refs_host.py, for the 27 walks of libhsddp_hip.so)."""
    import test_refs_host as tr
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc")], stdout=subprocess.DEVNULL)
    d = os.path.join(ROOT, "cafe-mpc_amd")
    short = lambda ks: sorted(re.search(r"k_[a-z0-9_]+?(?=E[PN])", k).group(0) for k in ks)
    assert short(tr.gfx950_kernels(os.path.join(d, "libhsddp_fric.so"), tmp_path)) == ["k_sim_quad_fric", "k_sim_quad_mc0_fric", "k_sim_quad_mc_fric"]
    assert not [k for k in tr.gfx950_kernels(os.path.join(d, "libhsddp_hip.so"), tmp_path) if "fric" in k]
    dyn = subprocess.run(["readelf", "-d", os.path.join(d, "libhsddp_hip.so")], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhsddp_fric\.so\]", dyn) and re.search(r"(RUNPATH|RPATH).*\$ORIGIN", dyn)
    src = open(os.path.join(d, "csrc", "hsddp_hip.hip")).read()
    assert re.search(r'#ifndef HS_FRIC_SEPARATE[^\n]*\n#include "hsddp_fric.hip"\n#endif', src)


def test_make_resources_fric():
    """The conditions on the product build: the three kernels at one wave per SIMD with at most 40 KiB of LDS, and no scratch in the two without the
    generator.  The noisy twin's scratch, the registers and the spills are printed (DESIGN.md holds them beside the _ter twins')."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources-fric"], capture_output=True, text=True, check=True).stdout
    t, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        if m.group(1).startswith("Function Name: "):
            name = re.search(r"k_sim_quad[a-z0-9_]*fric", m.group(1)).group(0); t[name] = []
        else:
            t[name].append(m.group(1))
    assert sorted(t) == ["k_sim_quad_fric", "k_sim_quad_mc0_fric", "k_sim_quad_mc_fric"]
    for k, v in t.items():
        print("[fric]", k, "; ".join(v))
        assert "Occupancy [waves/SIMD]: 1" in v, k
        lds = [int(x.split(":")[1]) for x in v if x.startswith("LDS Size")]
        assert len(lds) == 1 and 0 < lds[0] <= 40 * 1024, (k, lds)
        scratch = [int(x.split(":")[1]) for x in v if x.startswith("ScratchSize")]
        assert len(scratch) == 1 and (k == "k_sim_quad_mc_fric" or scratch[0] == 0), (k, scratch)


def test_multiphase_ddp_header_compiles_with_friction(tmp_path):
    """The C++ mirror: Simulation::set_friction / friction and Episode::set_friction / friction compile, and so does the harness tests/cpp/friction_loop.cpp."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0, const int* mu_of) {\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8, true); std::vector<hsddp_friction_row_t> rows(8);\n'
                   '    hsddp_friction_t p = {0.02, 2, 0}; const double mu[4] = {1e9, 1e9, 0.6, 0.5};\n'
                   '    bool ok = sim.set_contact(true, -10.0, 0.0) && sim.set_friction(true, &p, mu, mu_of) && sim.run(x0) && sim.friction(rows.data()) && sim.set_friction(false);\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.set_contact(true, 0.0) && e.set_friction(true, &p, mu) && e.set_friction(false); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "friction_loop.cpp"), "-o", str(tmp_path / "l.o")])      # (linked and run in tests/test_friction_gpu.py)
