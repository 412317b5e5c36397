"""CPU tests of the sub-stepped integration (include/hsddp_substep.h): the ctypes mirror, the numpy statement sim.grf_rows_sub against
sim.grf_rows, and the sub-stepped program itself (cafe-mpc_amd/csrc/wb_sim.hpp with the SUB policies) compiled for the host by
tests/_emu/sub_emu.cpp - with one substep against the program without the switch, with several against the reference walk of tests/sub_common.py,
and its order of convergence.  Real HIP: tests/test_substep_gpu.py."""
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

MU = 0.6


def test_substep_abi_mirror_matches_the_header():
    """Every prototype of include/hsddp_substep.h is in SUBSTEP_EXPORTS and in no other list; bind_substep refuses a library that lacks one; the
    lists and binders of the other headers are what they were."""
    src = open(os.path.join(ROOT, "include", "hsddp_substep.h")).read()
    protos = set(re.findall(r"\b(hsddp_substep_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    A = pkg._abi
    assert protos == set(A.SUBSTEP_EXPORTS) and len(protos) == 2
    others = set(A.EXPORTS) | set(A.ENSEMBLE_EXPORTS) | set(A.HKD_EXPORTS) | set(A.REFS_EXPORTS) | set(A.SIM_EXPORTS) | set(A.MC_EXPORTS) | set(A.GRF_EXPORTS) | set(A.EPISODE_EXPORTS)
    assert not protos & others
    assert (len(A.SIM_EXPORTS), len(A.MC_EXPORTS), len(A.GRF_EXPORTS), len(A.EPISODE_EXPORTS)) == (7, 2, 2, 9)
    assert int(re.search(r"#define HSDDP_SUBSTEP_MAX (\d+)", src).group(1)) == A.SUBSTEP_MAX == 64

    class Fake:
        pass
    lib = Fake()
    for s in A.SIM_EXPORTS + A.SUBSTEP_EXPORTS[:-1]:
        setattr(lib, s, Fake())
    with pytest.raises(RuntimeError):
        A.bind_substep(lib)
    setattr(lib, A.SUBSTEP_EXPORTS[-1], Fake())
    A.bind_substep(lib)
    assert lib.hsddp_substep_set.argtypes == [ctypes.c_void_p, ctypes.c_int] and len(lib.hsddp_substep_get.argtypes) == 2
    old = Fake()      # a library with the symbols of the earlier headers alone still binds through every earlier binder
    for s in A.SIM_EXPORTS + A.MC_EXPORTS + A.GRF_EXPORTS + A.EPISODE_EXPORTS:
        setattr(old, s, Fake())
    A.bind_episode(old)
    with pytest.raises(RuntimeError):
        A.bind_substep(old)


def test_grf_rows_sub_is_grf_rows_on_the_flattened_substeps():
    """Hand-made forces, n = 3 control steps x S = 4 substeps: a violation in substep 2 of step 1 only, a `counted` mask that ends inside step 2,
    a swing foot that is ignored; the row equals grf_rows of the n S flattened steps with the contact rows repeated and first_slip // S."""
    n, S, mu = 3, 4, 0.5
    contact = np.array([[1, 0, 0, 1]] * n)
    Y = np.zeros((n, S, 12))
    Y[..., 0:3] = (1.0, -2.0, 10.0); Y[..., 9:12] = (0.0, 4.0, 12.0)      # both stance feet inside (cone 3 and 2)
    Y[..., 3:6] = (100.0, 100.0, -100.0)                                   # a swing foot's entries are not looked at
    Y[1, 2, 0:3] = (0.0, 6.0, 10.0)                                        # FL outside in substep 2 of step 1 only (cone -1)
    Y[2, 3, 9:12] = (0.0, 0.0, -3.0)                                       # HR pulls in the last substep of step 2
    Y[0, 1, 11] = 30.0

    def flat(Y, counted=None):
        Yf = Y.reshape(Y.shape[:-3] + (n * S, 12))
        if counted is None:
            ref = pkg.sim.grf_rows(Yf, np.repeat(contact, S, axis=0), mu, 0.0)
        else:      # a mask that is a prefix of the flattened steps is grf_rows' first_bad rule
            cnt = counted.reshape(counted.shape[:-2] + (n * S,))
            nb = cnt.sum(axis=-1)
            assert np.array_equal(cnt, np.arange(n * S) < nb[..., None])
            ref = pkg.sim.grf_rows(Yf, np.repeat(contact, S, axis=0), mu, 0.0, first_bad=np.where(nb == n * S, -1, nb - 1))
        ref = ref.copy()
        ref["first_slip"] = np.where(ref["first_slip"] >= 0, ref["first_slip"] // S, -1)
        return ref
    r = pkg.sim.grf_rows_sub(Y, contact, mu, 0.0)
    assert r.shape == () and r.dtype == pkg._abi.GRF_ROW_DTYPE and r.tobytes() == flat(Y).tobytes()
    assert (r["min_fz"], r["min_cone"], r["max_fz"], r["first_slip"], r["n_slip"]) == (-3.0, -1.5, 30.0, 1, 2)
    # the mask ends mid-step: substeps 0 and 1 of step 2 count, the pulling substep 3 does not
    counted = np.ones((n, S), dtype=bool); counted[2, 2:] = False
    c = pkg.sim.grf_rows_sub(Y, contact, mu, 0.0, counted=counted)
    assert c.tobytes() == flat(Y, counted).tobytes() and (c["min_fz"], c["first_slip"], c["n_slip"]) == (10.0, 1, 1)
    # leading axes, one mask per sample: everything / up to the violating substep inclusive / short of it / nothing
    YY = np.stack([Y] * 4)
    cc = np.ones((4, n, S), dtype=bool); cc[1, 1, 3:] = False; cc[1, 2] = False; cc[2, 1, 2:] = False; cc[2, 2] = False; cc[3] = False
    m = pkg.sim.grf_rows_sub(YY, contact, mu, 0.0, counted=cc)
    assert m[:3].tobytes() == flat(YY[:3], cc[:3]).tobytes()
    assert list(m["first_slip"]) == [1, 1, -1, -1] and list(m["n_slip"]) == [2, 1, 0, 0] and m["min_fz"][3] == np.inf and m["max_fz"][3] == -np.inf
    # S = 1 is grf_rows itself
    assert pkg.sim.grf_rows_sub(Y[:, :1], contact, mu, 0.0).tobytes() == pkg.sim.grf_rows(Y[:, 0], contact, mu, 0.0).tobytes()


@pytest.fixture(scope="module")
def sub_emu(tmp_path_factory):
    return sub.build_emu(tmp_path_factory.mktemp("sub_emu"))


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


def host_run(lib, so, xs, smap, S, d=None, k=None, mu=0.0):
    outs = [sub.emu_run(lib, pkg, so, b, xs[b], smap, S, d, None if k is None else k[b], mu) for b in range(xs.shape[0])]
    return outs, sub.emu_result(pkg, outs, d is not None or k is not None, mu > 0)


@pytest.mark.parametrize("case", ["plain", "D", "records"])
def test_one_substep_on_the_host_is_the_walk_without_the_switch(sub_emu, solved_trot, case):
    """The SUB program with S = 1 (dt / 1 is dt; one trip, then the impact) against the program without the switch, 48 steps: every output bit for
    bit.  (The library launches the kernels without the switch for S = 1; this holds the SUB walk itself to them.)"""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 48)
    d, k = mc.cases(pkg, xs.shape[:2])["D"] if case == "D" else (None, None)
    mu = MU if case == "records" else 0.0
    one, _ = host_run(sub_emu, so, xs, smap, 1, d, k, mu)
    off, _ = host_run(sub_emu, so, xs, smap, 0, d, k, mu)
    for a, b in zip(one, off):
        for f in a:
            assert a[f].tobytes() == b[f].tobytes(), (case, f)
    assert np.abs(one[0]["X"]).max() > 0.1 and (case != "records" or np.abs(one[0]["Y"]).max() > 1.0) and (case != "D" or one[0]["extra"][:, 1].sum() > 0)


PARITY = [("plain", 3), ("plain", 4), ("A", 3), ("C", 4), ("D", 4), ("records", 4)]


@pytest.mark.parametrize("n_steps", [48, 24])
@pytest.mark.parametrize("case,S", PARITY)
def test_substepped_program_on_the_host_matches_the_reference(sub_emu, oracle_lib, solved_trot, case, S, n_steps):
    """Trot 4 x 12, 4 problems x 8 samples, 48 steps (a lift-off and both reset maps) and 24: plain at S = 3 and 4, case A at S = 3, cases C and D
    at S = 4, records at S = 4 with mu = 0.6 (margins of the reference: min |cone| 4.0e-3 N against 6.6e-4 N needed; S = 2 would give 7.6e-4 N and
    is not used for the exact counts).  The run differs from the S = 1 walk by 0.2 - 1.0 against a bound of about 1e-7."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, n_steps)
    d, k = mc.cases(pkg, xs.shape[:2])[case] if case in "ABCD" else (None, None)
    mu = MU if case == "records" else 0.0
    ref = sub.oracle_walk_sub(pkg, oracle_lib, phases, pol, smap, xs, S, d, k)
    assert (ref["first_bad"] == -1).all() and ref["counted"].all()
    if d is not None:
        assert not ((ref["sat_margin"] < mc.NEAR) | (ref["fall_margin"] < mc.NEAR)).any()      # the reference alone leaves no sample out
    outs, res = host_run(sub_emu, so, xs, smap, S, d, k, mu)
    sub.compare_case(f"host {case} S={S} n={n_steps}", pkg, res, ref, mc.xbar_window(pol, smap), gc.contact_of(phases, smap), mu, 0.0)
    _, base = host_run(sub_emu, so, xs[:1], smap, 1, d, None if k is None else k[:1], mu)
    gap = float(np.abs(base["X"] - res["X"][:1]).max())
    print(f"[sub] host {case} S={S} n={n_steps}: largest |X(S) - X(1)| of problem 0 = {gap:.3f}")
    assert gap > 1e-3      # the finer integrator does move the closed loop
    if case == "records":
        plain = host_run(sub_emu, so, xs, smap, S)[1]
        for f in ("x_final", "X", "U"):
            assert np.array_equal(res[f], plain[f]), f
        assert res["rows"].tobytes() == plain["rows"].tobytes()
        lean = sub.emu_run(sub_emu, pkg, so, 1, xs[1], smap, S, mu=mu, keep_traj=False)
        assert np.array_equal(lean["g"], outs[1]["g"]) and np.isnan(lean["Y"]).all()


def test_substepped_program_on_the_host_is_first_order(sub_emu, solved_trot):
    """2 problems x 2 samples, the first 12 steps (one stance phase, no impact): |x_final(S) - x_final(64)|inf for S = 1, 2, 4, 8 has consecutive
    ratios in [1.6, 2.6] - forward Euler under a held torque is first order (the reference alone gives 2.02, 2.06, 2.14)."""
    phases, so, xs, pol = solved_trot
    smap = sc.step_map(phases, 12)
    assert not smap[2].any()
    fin = {S: host_run(sub_emu, so, xs[:2, :2], smap, S)[1]["x_final"] for S in (1, 2, 4, 8, 64)}
    err = [float(np.abs(fin[S] - fin[64]).max()) for S in (1, 2, 4, 8)]
    ratios = [err[i] / err[i + 1] for i in range(3)]
    print(f"[sub] errors against S = 64: {['%.3e' % e for e in err]}, ratios {['%.3f' % r for r in ratios]}")
    assert all(1.6 <= r <= 2.6 for r in ratios), ratios


def test_multiphase_ddp_header_compiles_with_substeps(tmp_path):
    """The C++ mirror: Simulation::set_substeps / substeps and Episode::set_substeps compile."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* x0) {\n'
                   '    hsddp::Simulation sim(s.handle(), 2, 4, 8, true); bool ok = sim.set_substeps(4) && sim.substeps() == 4 && sim.run(x0) && sim.set_substeps(1);\n'
                   '    hsddp::Episode e(s.handle(), 2, 4, 3); ok = ok && e.set_substeps(4) && e.set_grf(0.6); (void)ok;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
