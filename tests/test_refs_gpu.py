"""Per-problem tracking references (include/hsddp_refs.h) on the device: explicit shared values change nothing, a command ensemble in one handle
equals one batch-1 handle per command bit for bit (and the oracle at the parity tolerances), partial ranges, read-back, device sources, a
fleet MPC loop over reconfigure, and the argument checks."""
import importlib
import os

import numpy as np
import pytest

from conftest import pkg, ROOT
import parity_common as pc

pytestmark = pytest.mark.gpu

TREE = os.path.join(ROOT, "tests", "golden", "cafe_tree")
builder = importlib.import_module(pkg.__name__ + ".builder")
P = pkg.problems
FIELDS = ("X", "XBAR", "U", "UBAR", "K", "Y")
SPEEDS = np.linspace(0.0, 0.7, 8)
EINVAL = -1


def make(lib, phases, x0, nominal=None, refs=None, **kw):
    """Solver on `phases` with per-problem nominal [(Xbar [B,h+1,n], Ubar [B,h,m]) per phase] and per-problem references (stack_references)."""
    s = pkg.Solver(lib, phases, batch=x0.shape[0], **kw)
    for i, p in enumerate(phases):
        if nominal is None:
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        else:
            s.set_nominal(i, *nominal[i])
    if refs is not None:
        for i, r in enumerate(refs):
            s.set_references(i, **r)
    s.set_initial_condition(x0)
    return s


def stacked_nominal(lists):
    return [(np.stack([pl[i]["Xbar"] for pl in lists]), np.stack([pl[i]["Ubar"] for pl in lists])) for i in range(len(lists[0]))]


def assert_problem_equal(sa, a, sb, b, tag=""):
    """Problem a of handle sa and problem b of handle sb: info and every field bit-identical."""
    ia, ib = sa.info_arrays(), sb.info_arrays()
    for k in ia:
        assert np.array_equal(ia[k][a], ib[k][b], equal_nan=True), (tag, k, ia[k][a], ib[k][b])
    for i in range(len(sa.phases)):
        for f in FIELDS:
            x, y = sa.field(i, f, a, 1), sb.field(i, f, b, 1)
            assert np.array_equal(x, y, equal_nan=True), (tag, i, f, np.abs(x - y).max() if x.size else 0)


def assert_handles_equal(sa, sb, problems, tag=""):
    for b in problems:
        assert_problem_equal(sa, b, sb, b, tag)


@pytest.mark.parametrize("ms", [1, 0])
def test_explicit_shared_references_change_nothing(hip_lib, ms):
    phases = P.wb_trot_problem()
    x0 = P.wb_ensemble_x0(8, 20260101)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3, MS=ms)
    plain = make(hip_lib, phases, x0)
    refs = P.stack_references([phases] * 8)
    explicit = make(hip_lib, phases, x0, refs=refs)
    plain.solve(opt); explicit.solve(opt)
    assert_handles_equal(plain, explicit, range(8), f"MS={ms}")
    plain.close(); explicit.close()


def ensemble_case(name):
    if name == "wb":
        lists = [P.wb_trot_problem(vx=v) for v in SPEEDS]
        return lists, P.wb_ensemble_x0(8, 20260102), pkg.PREC_F64, pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3)
    if name == "mhpc":
        lists = [P.mhpc_problem(vx=v) for v in SPEEDS]
        return lists, P.wb_ensemble_x0(8, 20260103), pkg.PREC_F64, pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3)
    lists = [P.hkd_trot_problem(vx=v) for v in SPEEDS]
    prec = pkg.PREC_F32 if name == "hkd_f32" else pkg.PREC_F64
    return lists, P.hkd_ensemble_x0(8, 20260104, lists[0]), prec, P.hkd_ddp_setting()


@pytest.mark.parametrize("name", ["wb", "mhpc", "hkd_f64", "hkd_f32"])
def test_command_ensemble_equals_single_handles(hip_lib, name):
    lists, x0, prec, opt = ensemble_case(name)
    s = make(hip_lib, lists[0], x0, nominal=stacked_nominal(lists), refs=P.stack_references(lists), precision=prec)
    s.solve(opt)
    for b, pl in enumerate(lists):
        one = make(hip_lib, pl, x0[b:b + 1], precision=prec)
        one.solve(opt)
        assert_problem_equal(s, b, one, 0, f"{name} speed {SPEEDS[b]}")
        one.close()
    assert len(set(np.round(s.info_arrays()["actual_cost"], 12))) > 1      # the commands really differ
    s.close()


class ProblemView:
    """One problem of a batched handle, seen as a batch-1 solver (for parity_common.compare_solve)."""

    def __init__(self, s, b):
        self.s, self.b = s, b

    def info_arrays(self):
        return {k: v[self.b:self.b + 1] for k, v in self.s.info_arrays().items()}

    def field(self, phase, name):
        return self.s.field(phase, name, self.b, 1)


def test_command_ensemble_oracle_parity(hip_lib, oracle_lib):
    """test_full_solve_parity_trot's problem and tolerances, one command per problem of the batched handle."""
    lists = [P.wb_trot_problem(horizons=(12, 12, 12, 12), vx=v) for v in SPEEDS]
    x0 = P.wb_ensemble_x0(8, 20241222)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=3, max_DDP_iter=4)
    s = make(hip_lib, lists[0], x0, nominal=stacked_nominal(lists), refs=P.stack_references(lists))
    s.solve(opt)
    for b in (0, 3, 7):
        so = make(oracle_lib, lists[b], x0[b:b + 1])
        so.solve(opt)
        pc.compare_solve(so, ProblemView(s, b), len(lists[b]))
        so.close()
    s.close()


def test_partial_range_and_read_back(hip_lib):
    phases = P.wb_trot_problem(horizons=(20, 20, 20, 20))
    other = P.wb_trot_problem(horizons=(20, 20, 20, 20), vx=0.2)
    x0 = P.wb_ensemble_x0(8, 20260105)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=3)
    shared = make(hip_lib, phases, x0)
    part = make(hip_lib, phases, x0)
    st = P.stack_references([other] * 3)
    for i in range(len(phases)):
        part.set_references(i, b0=2, **st[i])
    for i in range(len(phases)):
        got = part.get_references(i)
        for k, v in st[i].items():
            assert np.array_equal(got[k][2:5], v), (i, k)
            for b in (0, 1, 5, 6, 7):
                assert np.array_equal(got[k][b], phases[i]["bufs"][k]), (i, k, b)
        assert np.array_equal(part.get_references(i, b0=3, nb=2)["xr"], st[i]["xr"][1:3])
        assert np.array_equal(shared.get_references(i, b0=1, nb=2)["foot_pos"], np.stack([phases[i]["bufs"]["foot_pos"]] * 2))
    # a later call overwrites the given fields of its range only
    bp = st[0]["body_pos"][:1] + 1.0
    part.set_references(0, b0=3, body_pos=bp)
    g = part.get_references(0)
    assert np.array_equal(g["body_pos"][3], bp[0]) and np.array_equal(g["xr"][3], st[0]["xr"][1]) and np.array_equal(g["body_pos"][2], st[0]["body_pos"][0])
    part.set_references(0, b0=3, body_pos=st[0]["body_pos"][1:2])
    shared.solve(opt); part.solve(opt)
    assert_handles_equal(shared, part, (0, 1, 5, 6, 7), "outside the range")
    one = make(hip_lib, other, x0[2:3], nominal=[(p["Xbar"], p["Ubar"]) for p in phases])      # the nominal part was given
    one.solve(opt)
    assert_problem_equal(part, 2, one, 0, "inside the range")
    for s in (shared, part, one):
        s.close()


DEVICE_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")      # torch's runtime first, then the package's library
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package(); P = pkg.problems
lists = [P.hkd_trot_problem(vx=v) for v in np.linspace(0.0, 0.7, 8)]
x0 = P.hkd_ensemble_x0(8, 20260106, lists[0]); opt = P.hkd_ddp_setting()
refs = P.stack_references(lists)
out = {}
for kind in ("host", "device"):
    s = pkg.MultiPhaseDDP(lists[0], batch=8)
    for i in range(len(lists[0])):
        s.set_nominal(i, np.stack([pl[i]["Xbar"] for pl in lists]), np.stack([pl[i]["Ubar"] for pl in lists]))
        r = refs[i] if kind == "host" else {k: torch.from_numpy(v).to("cuda") for k, v in refs[i].items()}
        s.set_references(i, **r)
    if kind == "device":
        t = torch.from_numpy(refs[0]["xr"]).to("cuda")
        for bad in (t.float(), t.transpose(1, 2).contiguous().transpose(1, 2), t.cpu()):
            try:
                s.set_references(0, xr=bad); raise SystemExit("accepted a bad tensor")
            except ValueError:
                pass
    for i in range(len(lists[0])):
        for k, v in s.get_references(i).items():
            out[f"{kind}_refs_{i}_{k}"] = v
    s.set_initial_condition(x0); s.solve(opt)
    for k, v in s.info_arrays().items():
        out[f"{kind}_info_{k}"] = v
    for i in range(len(lists[0])):
        for f in ("X", "XBAR", "U", "UBAR", "K", "Y"):
            out[f"{kind}_{i}_{f}"] = s.field(i, f)
    s.close()
np.savez(sys.argv[2], **out)
"""


def test_device_sources_equal_host_sources(tmp_path):
    """Torch tensors on the handle's device (read in place) against the same values from numpy, in a process of its own: torch's HIP runtime
    has to be up before the package's library is loaded."""
    import subprocess
    import sys
    (tmp_path / "dev.py").write_text(DEVICE_SCRIPT)
    out = tmp_path / "out.npz"
    subprocess.check_call([sys.executable, str(tmp_path / "dev.py"), ROOT, str(out)], timeout=600)
    d = np.load(out)
    keys = [k[len("host_"):] for k in d.files if k.startswith("host_")]
    assert len(keys) > 20
    for k in keys:
        assert np.array_equal(d["host_" + k], d["device_" + k], equal_nan=True), k
    lists = [P.hkd_trot_problem(vx=v) for v in SPEEDS]
    assert np.array_equal(d["device_refs_2_xr"], np.stack([pl[2]["bufs"]["xr"] for pl in lists]))


# ------------------------------------------------------------------------------------------------ fleet MPC loop
def bound_problem_data():
    cp = builder.load_hkd_constraint_params(os.path.join(TREE, "HKDMPC/settings/constraint_params.info"))
    return builder.HKDProblemData(builder.QuadReference(os.path.join(TREE, "Reference/Data/bound/quad_reference.csv"), reorder=True), cp)


def ddp_setting(al, ddp):
    opt = builder.load_ddp_setting(os.path.join(TREE, "HKDMPC/settings/ddp_setting.info"))
    opt.max_AL_iter, opt.max_DDP_iter = al, ddp
    return opt


def translate_state(x, contact, dx, dy):
    """An HKD state moved like translate_references moves a reference row."""
    x = np.array(x, dtype=np.float64, copy=True)
    x[3:5] += (dx, dy)
    for l in range(4):
        if contact[l] > 0:
            x[12 + 3 * l:14 + 3 * l] += (dx, dy)
    return x


def reconfigure_with(solver, old_phases, new_phases, slot_map):
    """builder.shift_solver_in_place with the caller's descriptors (a robot's translated window)."""
    old_index = {p.get("uid"): i for i, p in enumerate(old_phases)}
    src = [old_index.get(p.get("uid"), -1) for p in new_phases]
    shift = [slot_map[p["uid"]][0] if s >= 0 else 0 for p, s in zip(new_phases, src)]
    solver.reconfigure(new_phases, src, shift)


def test_fleet_mpc_loop(hip_lib):
    offsets = [(0.0, 0.0), (1.5, -0.5), (-2.0, 3.0), (10.0, 7.25)]
    R = len(offsets)
    pd = bound_problem_data()
    phases, info = pd.describe()
    moved = [P.translate_references(phases, dx, dy) for dx, dy in offsets]
    c0 = phases[0]["bufs"]["ref_contact"][0]
    x0 = np.stack([translate_state(info["x0"], c0, dx, dy) for dx, dy in offsets])
    x0[:, :12] += np.random.default_rng(7).uniform(-0.01, 0.01, (R, 12))
    opt0, opt_rt = ddp_setting(2, 4), ddp_setting(2, 1)
    fleet = make(hip_lib, moved[0], x0, nominal=stacked_nominal(moved), refs=P.stack_references(moved))
    singles = [make(hip_lib, moved[r], x0[r:r + 1]) for r in range(R)]
    for s in [fleet] + singles:
        s.solve(opt0)
    for r in range(R):
        assert_problem_equal(fleet, r, singles[r], 0, f"tick 0 robot {r}")
    mallocs, ph, mv = [], phases, moved
    for tick in range(1, 11):
        m = pd.update()
        new, _ = pd.describe()
        new_mv = [P.translate_references(new, dx, dy) for dx, dy in offsets]
        reconfigure_with(fleet, ph, new, m)
        for i, r in enumerate(P.stack_references(new_mv)):
            fleet.set_references(i, **r)
        for r in range(R):
            reconfigure_with(singles[r], mv[r], new_mv[r], m)
        for s in [fleet] + singles:
            s.set_control_knot(0, 0, None)
            s.set_initial_condition(np.ascontiguousarray(s.field(0, "XBAR")[:, 0]))
            s.solve(opt_rt)
        for r in range(R):
            assert_problem_equal(fleet, r, singles[r], 0, f"tick {tick} robot {r}")
        ph, mv = new, new_mv
        mallocs.append(hip_lib.hsddp_debug_malloc_count())
    assert mallocs[3:] == [mallocs[3]] * len(mallocs[3:]), mallocs      # flat from tick 4 on
    for s in [fleet] + singles:
        s.close()


def test_argument_checks(hip_lib):
    pkg._abi.bind_refs(hip_lib)
    phases = P.mhpc_problem(wb_horizons=(10, 10), srb_horizons=(4, 4))     # WB (p = 12) then SRB (p = 0)
    x0 = P.wb_ensemble_x0(4, 20260107)
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    s = make(hip_lib, phases, x0)
    ref = make(hip_lib, phases, x0)
    st = P.stack_references([phases] * 4)
    refs = pkg._abi.Refs()
    keep = {k: np.ascontiguousarray(v + (0.5 if v.dtype == np.float64 else 0)) for k, v in st[0].items()}
    for k, v in keep.items():
        setattr(refs, k, v.ctypes.data)
    call = lambda ph, b0, nb, r=refs: hip_lib.hsddp_set_references(s.h, ph, b0, nb, ctypes_byref(r), 0)
    for ph, b0, nb in ((-1, 0, 1), (len(phases), 0, 1), (0, -1, 1), (0, 0, 5), (0, 3, 2), (0, 4, 1), (0, 0, 0), (0, 0, -1)):
        assert call(ph, b0, nb) == EINVAL, (ph, b0, nb)
    srb = pkg._abi.Refs(); yr = np.zeros((1, 5, 12)); srb.yr = yr.ctypes.data
    assert call(2, 0, 1, srb) == EINVAL                                     # yr on a phase with p = 0
    out = np.zeros((1, 5, 12))
    assert hip_lib.hsddp_get_references(s.h, 2, 0, 1, None, None, out.ctypes.data, None, None, None, None) == EINVAL
    assert hip_lib.hsddp_get_references(s.h, 0, 3, 2, None, None, None, None, None, None, None) == EINVAL
    assert hip_lib.hsddp_set_references(s.h, 0, 0, 1, None, 0) == EINVAL
    with pytest.raises(ValueError):
        s.set_references(0, xr=np.zeros((1, 3, 36)))
    with pytest.raises(ValueError):
        s.set_references(0, bogus=np.zeros((1, 11, 36)))
    s.solve(opt); ref.solve(opt)
    assert_handles_equal(ref, s, range(4), "after refused calls")
    s.close(); ref.close()


def ctypes_byref(x):
    import ctypes
    return ctypes.byref(x)
