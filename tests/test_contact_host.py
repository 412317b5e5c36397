"""CPU tests of unilateral ground contact (include/hsddp_contact.h): the ctypes mirror, the reference walk of tests/uni_common.py on hand-checkable
properties, and the program itself (cafe-mpc_amd/csrc/wb_sim.hpp with the UNI policies) compiled for the host by tests/_emu/uni_emu.cpp against that
reference - without an event, with base kicks that send samples into free flight and back, with a roll kick under noise and a torque clip, on a
contained divergence, and over episode ticks with F handed over.  Plus make resources against the parent's.  Real HIP: tests/test_contact_gpu.py."""
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
import sub_common as sub
import uni_common as un

MU = 0.6


def test_contact_abi_mirror_matches_the_header():
    """Every prototype of include/hsddp_contact.h is in CONTACT_EXPORTS and in no other list; bind_contact refuses a library that lacks one; the row
    dtype has the layout of hsddp_contact_row_t; the lists of the other headers are what they were."""
    src = open(os.path.join(ROOT, "include", "hsddp_contact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = set(re.findall(r"\b(hsddp_contact_[a-z_]+)\s*\(", code))
    A = pkg._abi
    assert protos == set(A.CONTACT_EXPORTS) and len(protos) == 3
    others = set(A.EXPORTS) | set(A.ENSEMBLE_EXPORTS) | set(A.HKD_EXPORTS) | set(A.REFS_EXPORTS) | set(A.SIM_EXPORTS) | set(A.MC_EXPORTS) | set(A.GRF_EXPORTS) | set(A.EPISODE_EXPORTS) | set(A.SUBSTEP_EXPORTS)
    assert not protos & others
    assert (len(A.SIM_EXPORTS), len(A.MC_EXPORTS), len(A.GRF_EXPORTS), len(A.EPISODE_EXPORTS), len(A.SUBSTEP_EXPORTS)) == (7, 2, 2, 9, 2)
    body = re.search(r"typedef struct \{(.*?)\} hsddp_contact_row_t;", code, flags=re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(A.CONTACT_ROW_DTYPE.names) and A.CONTACT_ROW_DTYPE.itemsize == 32 and A.CONTACT_ROW_DTYPE.fields["max_lift"][1] == 24

    class Fake:
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.CONTACT_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_contact(lib)
    setattr(lib, A.CONTACT_EXPORTS[-1], Fake())
    A.bind_contact(lib)
    assert lib.hsddp_contact_set.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double] and len(lib.hsddp_contact_get_params.argtypes) == 4


@pytest.fixture(scope="module")
def uni_emu(tmp_path_factory):
    return un.build_emu(tmp_path_factory.mktemp("uni_emu"))


@pytest.fixture(scope="module")
def sub_emu(tmp_path_factory):
    return sub.build_emu(tmp_path_factory.mktemp("sub_emu_for_uni"))


@pytest.fixture(scope="module")
def solved_trot(oracle_lib):
    """The fixture of tests/test_mc_host.py: trot 4 x 12, four problems, 3 AL x 4 DDP iterations, eight samples around Xbar[0] (sigma 0.02 / 0.2)."""
    phases = pkg.problems.wb_trot_problem(horizons=(12, 12, 12, 12))
    so = pkg.Solver(oracle_lib, phases, batch=4)
    for i, p in enumerate(phases):
        so.set_nominal(i, p["Xbar"], p["Ubar"])
    so.set_initial_condition(pkg.problems.wb_ensemble_x0(4, 20241222)); so.solve(pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4))
    xs = pkg.problems.perturbed_states(so.field(0, "XBAR")[:, 0], 8, 0.02, 0.2, seed=20241222)
    yield phases, so, xs, mc.policy_of(so)
    so.close()


def test_no_event_on_the_host_is_the_bilateral_walk(uni_emu, sub_emu, oracle_lib, solved_trot):
    """Case 1: fz_rel = -1e9 never releases; S = 3 with records agrees with the bilateral sub-stepped program and with the bilateral reference in
    everything, and every new counter is 0."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    res = un.host_run(uni_emu, pkg, so, xs, smap, 3, -1e9, 0.0, mu=MU)
    outs = [sub.emu_run(sub_emu, pkg, so, b, xs[b], smap, 3, None, None, MU) for b in range(xs.shape[0])]
    base = sub.emu_result(pkg, outs, False, True)
    same = all(np.array_equal(res[f], base[f]) for f in ("X", "U", "x_final", "Y")) and res["rows"].tobytes() == base["rows"].tobytes() and res["grf"].tobytes() == base["grf"].tobytes()
    print(f"[uni] host no event: bit-identical to the bilateral program: {same}")
    ref = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs, 3)
    sub.compare_case("host uni no event S=3", pkg, res, ref, mc.xbar_window(pol, smap), gc.contact_of(phases, smap), MU, 0.0)
    c = res["contact"]
    assert (c["first_release"] == -1).all() and not c["n_release"].any() and not c["n_land"].any() and not c["n_free"].any() and not c["free_final"].any() and not c["max_lift"].any()


def test_reference_walk_without_an_event_is_the_bilateral_reference(oracle_lib, solved_trot):
    """The reference itself: with fz_rel = -1e9 it is sub_common.oracle_walk_sub, bit for bit; one solve per substep."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 24)
    a = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap, xs[:2, :3], 2, -1e9, 0.0)
    b = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs[:2, :3], 2)
    for f in ("X", "U", "Y"):
        assert np.array_equal(a[f], b[f]), f
    assert (a["solves"] == 48).all() and np.array_equal(a["att"][0, 0, :, 0], gc.contact_of(phases, smap) > 0)


@pytest.mark.parametrize("case,S", un.CASES)
def test_program_on_the_host_matches_the_reference(uni_emu, oracle_lib, solved_trot, case, S):
    """Cases 2, 3, 5 and 6 of uni_common.case_setup against the reference walk; the non-vacuity of each case is asserted on the REFERENCE, and so is
    the cap of one left-out sample, before anything is compared.  Then the invariants of the run's own outputs (case 4)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs)
    ref = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap, x0, S, fz_rel, zg, d, k)
    un.assert_case_is_not_vacuous(case, ref, gc.contact_of(phases, smap))
    res = un.host_run(uni_emu, pkg, so, x0, smap, S, fz_rel, zg, d, k, MU)
    un.compare_case(f"host {case} S={S}", pkg, res, ref, mc.xbar_window(pol, smap)[:x0.shape[0]], MU, 0.0, fz_rel)
    un.invariants(f"host {case} S={S}", res, fz_rel, gc.force_bound(ref["Y"]))


def test_amplification_through_the_event_windows(uni_emu, solved_trot):
    """A 1e-12 change of x0 through the 48-step windows of cases 2 and 3 on the host build, over the samples that keep their decisions: printed, and
    at least two orders below the tolerance the windows are held to, 1e-8 x max(1, |X|max) (sim_common.close)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    rng = np.random.default_rng(7)
    for case, S in un.CASES[:3]:
        x0, d, k, fz_rel, zg = un.case_setup(pkg, case, xs)
        a = un.host_run(uni_emu, pkg, so, x0, smap, S, fz_rel, zg, d, k, MU)
        b = un.host_run(uni_emu, pkg, so, x0 + 1e-12 * rng.uniform(-1.0, 1.0, x0.shape), smap, S, fz_rel, zg, d, k, MU)
        ints = ("first_release", "n_release", "n_land", "n_free", "free_final")
        same = np.all([a["contact"][f] == b["contact"][f] for f in ints], axis=0)
        assert (a["rows"]["first_bad"] < 0).all() and same.sum() >= same.size - 1
        ev = same & (a["contact"]["n_release"] > 0)
        amp = np.abs(a["X"][same] - b["X"][same]).max() / 1e-12
        amp_ev = np.abs(a["X"][ev] - b["X"][ev]).max() / 1e-12 if ev.any() else 0.0
        scale = max(1.0, float(np.abs(a["X"]).max()))
        print(f"[uni] amplification {case} S={S}: {amp:.1f} x over {int(same.sum())} samples, {amp_ev:.1f} x over the {int(ev.sum())} with events; |X|max {scale:.1f}, "
              f"tolerance / 1e-12 = {sc.RTOL * scale / 1e-12:.0f}")
        assert ev.any() and amp * 1e-12 <= 0.01 * sc.RTOL * scale, (case, S, amp)


def test_episode_ticks_on_the_host_hand_f_over(uni_emu, oracle_lib, solved_trot):
    """The program walked in two 24-step pieces with F handed over through its pointer equals the one 48-step run, bit for bit (a kick in the first
    piece leaves feet free at the hand-over, asserted); a held sample does not write its F back; and the reference started from that F agrees."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    x0, d, k, fz_rel, zg = un.case_setup(pkg, "flight", xs)
    d1 = pkg.sim.Disturbance(seed=d.seed, u_max=d.u_max, kick_step=20)
    b = 1
    whole = un.emu_run(uni_emu, pkg, so, b, x0[b], smap, 4, fz_rel, zg, d1, k[b], MU)
    F = np.zeros((x0.shape[1], 4))
    first = un.emu_run(uni_emu, pkg, so, b, x0[b], smap[:, :24], 4, fz_rel, zg, d1, k[b], MU, F=F)
    masks = (F * np.array([1, 2, 4, 8])).sum(axis=1)
    assert np.array_equal(masks, first["c"][:, 4]) and (masks[first["rows"][:, 4] < 0] > 0).any()      # a live sample ends the piece with a free foot
    F2 = F.copy()
    hold = np.zeros(x0.shape[1], dtype=np.int32); hold[3] = 1
    smap2 = np.ascontiguousarray(smap[:, 24:])
    d2 = pkg.sim.Disturbance(seed=d.seed, u_max=d.u_max)      # the same torque limit, no kick
    second = un.emu_run(uni_emu, pkg, so, b, first["xf"], smap2, 4, fz_rel, zg, d2, None, MU, F=F2, hold=hold)
    live = first["rows"][:, 4] < 0
    assert np.array_equal(second["xf"][live], whole["xf"][live]) and np.array_equal(second["c"][live, 4], whole["c"][live, 4])
    assert np.array_equal(F2[3], F[3]) and np.array_equal((F2 * np.array([1, 2, 4, 8])).sum(axis=1)[hold == 0], second["c"][hold == 0, 4])
    ref = un.oracle_walk_uni(pkg, oracle_lib, phases, pol, smap2, first["xf"][None].repeat(b + 1, axis=0), 4, fz_rel, zg, d2, F0=(F > 0.5)[None].repeat(b + 1, axis=0))
    near = un.near_samples("host hand-over", {kk: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for kk, v in ref.items()})[0] | ~live
    got = un.contact_rows_of(pkg, second["c"])
    for f in ("first_release", "n_release", "n_land", "n_free", "free_final"):
        assert np.array_equal(got[f][~near], ref["rows"][f][b][~near]), f
    ok = ~near & (ref["first_bad"][b] < 0)
    sc.close("host hand-over x_final", second["xf"][ok], ref["X"][b, ok, -1])


def test_make_resources_leaves_every_existing_kernel_alone():
    """Case 10: make resources of this tree against the parent commit's output (profiles/r11uni_kernel_resource_usage_parent.txt): every kernel the
    parent has reports the same registers, spills, scratch, LDS and occupancy; the three new kernels are there at one wave per SIMD.  Their scratch,
    spills and LDS are recorded in DESIGN.md, not asserted."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources"], capture_output=True, text=True, check=True).stdout

    def table(text):
        t, name = {}, None
        for line in text.splitlines():
            m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
            if not m:
                continue
            if m.group(1).startswith("Function Name: "):
                name = m.group(1)[len("Function Name: "):]; t[name] = []
            else:
                t[name].append(m.group(1))
        return t
    now, parent = table(out), table(open(os.path.join(ROOT, "profiles", "r11uni_kernel_resource_usage_parent.txt")).read())
    assert len(parent) > 30
    for kname, lines in parent.items():
        assert now.get(kname) == lines, kname
    new = {k: v for k, v in now.items() if k not in parent}
    assert sorted(re.search(r"k_sim_quad[a-z0-9_]*uni", k).group(0) for k in new) == ["k_sim_quad_mc0_uni", "k_sim_quad_mc_uni", "k_sim_quad_uni"]
    for k, v in new.items():
        print("[uni]", re.search(r"k_sim_quad[a-z0-9_]*uni", k).group(0), "; ".join(v))
        assert "Occupancy [waves/SIMD]: 1" in v, k


def test_multiphase_ddp_header_compiles_with_contact(tmp_path):
    """The C++ mirror: Simulation::set_contact / contact and Episode::set_contact compile."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n#include <vector>\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0) {\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8, true); std::vector<hsddp_contact_row_t> rows(8);\n'
                   '    bool ok = sim.set_contact(true, 0.0, 0.0) && sim.run(x0) && sim.contact(rows.data()) && sim.set_contact(false);\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.set_contact(true, 0.0) && e.set_contact(false); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
