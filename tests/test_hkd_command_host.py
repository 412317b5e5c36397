"""CPU tests of the HKD-MPC command export (include/hsddp_hkd.h): its symbols and wire layout, the numpy specification hkd_command.pack_rows
on the CPU checker's fields, and the contact durations the HKD builders (Python and C++) now track."""
import ctypes
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT

TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")
builder = importlib.import_module(pkg.__name__ + ".builder")
hkd_command = importlib.import_module(pkg.__name__ + ".hkd_command")


def bound_problem_data():
    cp = builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info"))
    return builder.HKDProblemData(builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True), cp)


def test_hkd_header_symbols_match_binding_list():
    hdr = open(os.path.join(ROOT, "include", "hsddp_hkd.h")).read()
    assert sorted(set(re.findall(r"\b(hsddp_[a-zA-Z_]+)\s*\(", hdr))) == sorted(pkg._abi.HKD_EXPORTS)
    assert not set(pkg._abi.HKD_EXPORTS) & set(pkg._abi.EXPORTS)


def test_hip_library_exports_the_hkd_symbols(oracle_lib):
    if not os.path.exists(pkg.HIP_LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc")])
    lib = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for s in pkg._abi.HKD_EXPORTS:
        assert hasattr(lib, s), s
    pkg._abi.bind_hkd(lib)
    with pytest.raises(RuntimeError):       # the CPU checker keeps the shared ABI only
        pkg._abi.bind_hkd(oracle_lib)


def test_header_layout_is_the_packed_lcm_struct(tmp_path):
    """The word offsets of hsddp_hkd.h (and of hkd_command.LAYOUT) are those of a packed C struct of the hkd_command_lcmt fields in
    declaration order: 1954 words, feedback at word 513."""
    names = ["N_MPCSTEPS", "MPC_TIMES", "CONTROLS", "BODY_STATE", "CONTACTS", "STATUS_TIMES", "FOOT_PLACEMENT", "FEEDBACK", "SOLVE_TIME"]
    members = ["N_mpcsteps", "mpc_times", "hkd_controls", "des_body_state", "contacts", "statusTimes", "foot_placement", "feedback", "solve_time"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\n#include "hsddp_hkd.h"\n'
                   "#pragma pack(push, 1)\nstruct m { int32_t N_mpcsteps; double mpc_times[10]; float hkd_controls[10][24]; float des_body_state[10][12];\n"
                   "  int32_t contacts[10][4]; double statusTimes[10][4]; float foot_placement[12]; float feedback[10][12][12]; float solve_time; };\n"
                   "#pragma pack(pop)\nint main(){ printf(\"%zu %d %d\\n\", sizeof(struct m), HSDDP_HKD_CMD_WORDS, HSDDP_HKD_MAX_STEPS);\n"
                   + "".join(f'  printf("%zu %d\\n", offsetof(struct m, {mb}), HSDDP_HKD_OFF_{n});\n' for n, mb in zip(names, members))
                   + "  return 0; }\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = [list(map(int, l.split())) for l in subprocess.check_output([str(exe)]).decode().split("\n") if l.strip()]
    assert lines[0] == [1954 * 4, 1954, 10]
    assert pkg._abi.HKD_CMD_WORDS == 1954 and pkg._abi.HKD_MAX_STEPS == 10
    for (byte_off, word_off), (name, off, w, dt, shape) in zip(lines[1:], hkd_command.LAYOUT):
        assert byte_off == 4 * word_off == 4 * off, name
        assert w * 4 == np.dtype(dt).itemsize * int(np.prod(shape, dtype=int)), name
    assert hkd_command.OFFSETS["feedback"] == 513 and sum(w for _, _, w, _, _ in hkd_command.LAYOUT) == 1954


@pytest.fixture(scope="module", params=["fixture", "short"])
def oracle_hkd(oracle_lib, request):
    """An HKD window on the CPU checker, batch 3 (perturbed initial states), after a short solve: the bound fixture's first window (every leg
    finds its next foothold) or the first 36 knots of problems.hkd_bound_problem (the front legs do not land: their footholds come from pf_in)."""
    if request.param == "fixture":
        phases, info = bound_problem_data().describe()
        x0 = np.vstack([info["x0"]] * 3); x0[1, :12] += 0.01; x0[2, 3:6] -= 0.02
    else:
        phases = pkg.problems.hkd_bound_problem(n_knots=36)
        info = dict(contacts=[list(p["desc"].contact) for p in phases], status_durations=np.arange(len(phases) * 4, dtype=np.float64).reshape(-1, 4) / 7)
        x0 = pkg.problems.hkd_ensemble_x0(3, 20241220, phases)
    s = pkg.Solver(oracle_lib, phases, batch=3)
    for i, p in enumerate(phases):
        s.set_nominal(i, p["Xbar"], p["Ubar"])
    s.set_initial_condition(x0)
    s.solve(short_opt())
    yield s, phases, info
    s.close()


def short_opt():
    opt = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info"))
    opt.max_AL_iter, opt.max_DDP_iter = 1, 2
    return opt


@pytest.mark.parametrize("n_steps", [1, 9, 10])
def test_pack_rows_on_oracle_fields(oracle_hkd, n_steps):
    s, phases, info = oracle_hkd
    rng = np.random.default_rng(7 + n_steps)
    pf = rng.standard_normal((3, 12)).astype(np.float32)
    st = info["status_durations"]
    rows = hkd_command.pack_rows(s, 0, 3, n_steps=n_steps, mpc_time=0.04, dt=0.01, status_times=st, pf=pf)
    assert rows.shape == (3, 1954) and rows.dtype == np.uint32
    d = hkd_command.decode(rows)
    walk = hkd_command.step_map([p["desc"].horizon for p in phases], n_steps)
    assert d["N_mpcsteps"].tolist() == [n_steps] * 3
    for k, (i, kk) in enumerate(walk):
        K = s.field(i, "K")[:, kk]                    # [3, 24, 24] in (row, col) order
        assert np.array_equal(d["feedback"][:, k], K[:, :12, :12].astype(np.float32))
        assert np.array_equal(d["hkd_controls"][:, k], s.field(i, "UBAR")[:, kk].astype(np.float32))
        assert np.array_equal(d["des_body_state"][:, k], s.field(i, "XBAR")[:, kk, :12].astype(np.float32))
        assert (d["contacts"][:, k] == np.array(info["contacts"][i])).all()
        assert np.array_equal(d["statusTimes"][:, k], np.broadcast_to(st[i], (3, 4)))       # doubles survive the two-word round trip
        assert (d["mpc_times"][:, k] == 0.04 + k * 0.01).all()
    for name in ("feedback", "hkd_controls", "des_body_state", "contacts", "statusTimes", "mpc_times"):
        assert not d[name][:, n_steps:].any(), name    # rows k >= n_steps are zero
    for b in range(3):
        found = builder.hkd_next_footholds(s, info["contacts"], problem=b)
        assert sorted(found) == ([0, 1, 2, 3] if len(phases) > 4 else [2, 3])
        for l in range(4):
            want = found[l] if l in found else pf[b, 3 * l:3 * l + 3]
            assert np.array_equal(d["foot_placement"][b, 3 * l:3 * l + 3], want), (b, l)
    assert (d["solve_time"] == np.float32(s.solve_time_ms())).all()
    one = hkd_command.decode(rows[1])
    assert one["N_mpcsteps"] == n_steps and np.array_equal(one["raw"], rows[1])


def test_pack_rows_refuses_short_windows_and_bad_steps(oracle_hkd):
    s, phases, info = oracle_hkd
    for n in (0, 11):
        with pytest.raises(ValueError):
            hkd_command.pack_rows(s, n_steps=n)
    assert hkd_command.step_map([3, 2], 5) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)] and hkd_command.step_map([3, 2], 6) is None


def test_status_durations_follow_the_reference_rules():
    """contact_durations of HKDProblem (HKDProblem.cpp:27-38, 57, 63, 162-167, pop_front_phase in HKDProblem.h:55-66) over 10 ticks of the bound
    fixture: a phase of the initial table gets status_dur at its start time, a phase appended by update() status_dur at the horizon end when
    it appears, and the value travels with its phase until the phase is popped."""
    pd = bound_problem_data()
    ref, tp = pd.ref, pd.ref.tp["status_dur"]
    _, info = pd.describe()
    sd = info["status_durations"]
    assert sd.dtype == np.float64 and sd.shape == (len(info["horizons"]), 4)
    for i, t in enumerate(info["start_times"]):
        assert np.array_equal(sd[i], tp[ref.index(np.float32(t))]), i
    dur_of = {u: sd[i] for i, u in enumerate(pd.uid)}
    appended = popped = 0
    for tick in range(10):
        k0 = ref.k_cur
        old = set(pd.uid)
        pd.update()
        _, info = pd.describe()
        sd = info["status_durations"]
        assert sd.shape == (len(pd.uid), 4)
        popped += len(old - set(pd.uid))
        for i, u in enumerate(pd.uid):
            if u in dur_of:
                assert np.array_equal(sd[i], dur_of[u]), (tick, u)
            else:      # appended during this update: the sample at the horizon end of one of its simulation steps
                cands = [tp[k + ref.index(pd.plan)] for k in range(k0, ref.k_cur + 1)]
                assert any(np.array_equal(sd[i], c) for c in cands), (tick, u)
                dur_of[u] = sd[i]; appended += 1
    assert appended and popped
    assert len({tuple(v) for v in dur_of.values()}) > 2      # the durations differ between phases


def test_cpp_builder_durations_match_python(tmp_path):
    """tests/cpp/hkd_mpc_loop.cpp in its builder-only mode (no device): per tick the C++ HkdProblemData table and contact durations, bit-identical
    to the Python builder's."""
    exe = tmp_path / "hkd_mpc_loop"
    if not os.path.exists(pkg.HIP_LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc")])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "hkd_mpc_loop.cpp"), "-L", os.path.join(ROOT, "cafe-mpc_amd"), "-lhsddp_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "cafe-mpc_amd"), "-o", str(exe)])
    out = json.loads(subprocess.check_output([str(exe), TREE, "bound", "builder", "10"], timeout=300))
    pd = bound_problem_data()
    assert len(out["tables"]) == 11
    for tick, table in enumerate(out["tables"]):
        if tick:
            pd.update()
        _, info = pd.describe()
        assert [r["h"] for r in table] == info["horizons"], tick
        assert [r["contact"] for r in table] == info["contacts"], tick
        assert np.array_equal(np.array([r["dur"] for r in table], dtype=np.float64), info["status_durations"]), tick
