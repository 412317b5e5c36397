"""CPU tests: the relaxed barrier on both of its branches and the parameter updates between augmented-Lagrangian iterations (cases:
tests/barrier_common.py), on the oracle, its long-double build and the lane emulator tests/_emu.

* test_step_inputs_qualify / test_update_inputs_qualify: the fp64 oracle sits within 0.05 x the plain tolerances of its long-double build - per
  iterate on the step cases; on the update cases the two builds take the same decisions (counts, status), agree on REB_DELTA and AL_SIGMA bit for
  bit and on the number of times every REB_EPS entry was multiplied, and compare_solve holds at 0.05 x its tolerances.  The same through the
  window shift of wb_updates and the solve after it.
* test_step_coverage / test_update_coverage: the inputs reach what they are for.  Conditions, asserted from the oracle's fields.
* test_constraint_statement: barrier_common.constraint_values against the oracle: min(0, min g) over the window is max_pconstr, to 1e-12.
* test_emulator_matches_oracle: the kernel programs (one-wave knot, lane quad) on every step case against the oracle, per iterate, at the plain
  tolerances (1e-8 x scale, K 1e-6 absolute, scalars 1e-10), without the conditioning arbiter.

The emulator has no solve: k_update_params and the parameter copy of the reconfigure kernel run on the device only
(tests/test_barrier_gpu.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
import barrier_common as bc
import parity_common as pc

QUALIFY = 0.05


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "_emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    return pkg._abi.bind(ctypes.CDLL(os.path.join(d, "libhsddp_emu.so")))


# ------------------------------------------------------------------------------------------------------------- step cases
@pytest.mark.parametrize("name", bc.STEP_CASES)
def test_step_inputs_qualify(oracle_lib, oracle_ld_lib, name):
    phases, x0 = bc.step_case(name)
    so, sx = bc.make(oracle_lib, phases, x0), bc.make(oracle_ld_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, sx, phases, bc.step_option(name), n_iter=2, rtol=QUALIFY * 1e-8, atol_K=QUALIFY * 1e-6)
        print(f"[barrier] qualify {name}: oracle-vs-long-double / (0.05 x tolerance) {bc.worst_ratio(report)}")
    finally:
        so.close(); sx.close()


@pytest.fixture(scope="module")
def first_iterate(oracle_lib):
    """name -> (phases, G, D, max_pconstr per iterate, numpy's min(0, min g) per iterate) of the oracle: g and delta of the first iterate, the two
    scalars on both iterates."""
    cache = {}

    def get(name):
        if name not in cache:
            phases, x0 = bc.step_case(name)
            opt = bc.step_option(name)
            s = bc.make(oracle_lib, phases, x0)
            try:
                got, want, first = [], [], None
                for it in range(2):
                    s.hybrid_rollout(0.0 if it == 0 else 1.0, opt); s.compute_cost(opt)
                    G, D = bc.oracle_constraints(s)
                    first = first or (G, D)
                    got.append(s.info_arrays()["max_pconstr"].copy())
                    want.append(np.minimum(0.0, np.min([g.reshape(g.shape[0], -1).min(axis=1) for g in G], axis=0)))
                    if it == 0:
                        s.update_nominal_trajectory(); s.LQ_approximation(opt)
                        assert s.backward_sweep(0.0).all()
                        s.linear_rollout(1.0, opt)
            finally:
                s.close()
            cache[name] = (phases, first[0], first[1], got, want)
        return cache[name]
    return get


def _cells(cov, family):
    return {(k[1], k[2]): v for k, v in cov.items() if k[0] == family}


@pytest.mark.parametrize("name", bc.STEP_CASES)
def test_step_coverage(first_iterate, name):
    phases, G, D, _, _ = first_iterate(name)
    cov = bc.coverage(phases, G, D)
    full = dict(wb_edges=(("torque", 24), ("jointspeed", 24), ("joint", 24), ("height", 1)), hkd_edges=(("pyramid", 20),), srb_edges=(("height", 1),)).get(name, ())
    for family, count in full:      # the inputs set these values directly: no cell may be left out
        cells = _cells(cov, family)
        missing = [(i, r) for i in range(count) for r in bc.REGIONS if not cells.get((i, r))]
        assert not missing, (name, family, missing)
    if name == "wb_edges":
        # mixed waves: the plain problem's knots sit above every delta of the four families, beside problems that do not
        plain = 6
        for i, p in enumerate(phases):
            lay = bc.layout(p["desc"])
            cols = [c for c, (fam, _, _) in enumerate(lay) if fam != "grf"]
            assert (G[i][plain][:, cols] > D[i][plain][:, cols]).all(), i
    if name == "wb_grf_edges":
        cells = _cells(cov, "grf")
        rows = {(r, reg): sum(len(v) for (i, rg), v in cells.items() if i % 5 == r and rg == reg) for r in range(5) for reg in ("inside", "violated")}
        ranks = {rank: sum(len(v) for (i, rg), v in cells.items() if i // 5 == rank and rg != "above") for rank in range(4)}
        print(f"[barrier] coverage wb_grf_edges: (row, region) -> entries {rows}; rank -> entries inside or violated {ranks}")
        missing = [k for k, v in rows.items() if v == 0 and k not in bc.GRF_UNCOVERED]
        assert not missing, missing
        assert all(rows[k] == 0 for k in bc.GRF_UNCOVERED), "a cell listed as unreachable is reached: take it off the list"
        assert all(v > 0 for v in ranks.values()), ranks
    table = {}
    for (fam, idx, reg), v in cov.items():
        table.setdefault(fam, {r: 0 for r in bc.REGIONS})[reg] += len(v)
    print(f"[barrier] coverage {name}: entries with margin per family and region {table}")


@pytest.mark.parametrize("name", bc.STEP_CASES)
def test_constraint_statement(first_iterate, name):
    _, _, _, got, want = first_iterate(name)
    for it in range(2):
        assert (want[it] < 0).any(), (name, it, "no violated entry: the comparison would be 0 == 0")
        assert np.abs(got[it] - want[it]).max() <= 1e-12, (name, it, got[it], want[it])


EMU_CASES = [(n, "wave") for n in bc.STEP_CASES] + [(n, "quad") for n in bc.STEP_CASES if n.startswith("wb")]      # the lane quad is a whole-body program


@pytest.mark.parametrize("name,program", EMU_CASES, ids=[f"{n}-{p}" for n, p in EMU_CASES])
def test_emulator_matches_oracle(emu_lib, oracle_lib, monkeypatch, name, program):
    if program == "quad":
        monkeypatch.setenv("HSDDP_EMU_QUAD", "1")
    else:
        monkeypatch.delenv("HSDDP_EMU_QUAD", raising=False)
    phases, x0 = bc.step_case(name)
    so, se = bc.make(oracle_lib, phases, x0), bc.make(emu_lib, phases, x0)
    try:
        report = pc.run_steps(pkg, so, se, phases, bc.step_option(name), n_iter=2)
        print(f"[barrier] emulator {program} {name}: error / tolerance {bc.worst_ratio(report)}")
    finally:
        so.close(); se.close()


# ------------------------------------------------------------------------------------------------------------- update cases
@pytest.fixture(scope="module")
def update_solves(oracle_lib, oracle_ld_lib):
    """(name, max_AL_iter) -> (phases, x0, oracle handle, long-double handle), solved once."""
    cache = {}

    def get(name, n_al):
        if (name, n_al) not in cache:
            phases, x0, option = bc.update_case(name)
            so, sx = bc.make(oracle_lib, phases, x0), bc.make(oracle_ld_lib, phases, x0)
            so.solve(option(n_al)); sx.solve(option(n_al))
            cache[(name, n_al)] = (phases, x0, so, sx)
        return cache[(name, n_al)]
    yield get
    for _, _, so, sx in cache.values():
        so.close(); sx.close()


def _builds_agree(tag, phases, x0, so, sx, from_initial=True):
    io, ix = so.info_arrays(), sx.info_arrays()
    for k in pc.COUNT_KEYS:
        assert np.array_equal(io[k], ix[k]), (tag, k, io[k], ix[k])
    assert (io["status"] == 0).all(), (tag, io["status"])
    po, px = bc.params(so), bc.params(sx)
    init = bc.initial_params(phases, x0.shape[0])
    for i in range(len(phases)):
        assert np.array_equal(po["REB_DELTA"][i], px["REB_DELTA"][i]), (tag, "REB_DELTA", i)
        assert np.array_equal(po["AL_SIGMA"][i], px["AL_SIGMA"][i]), (tag, "AL_SIGMA", i)
        if po["REB_EPS"][i].size and from_initial:      # (after a shift the entries start from carried values: REB_DELTA speaks for the decisions)
            assert np.array_equal(bc.eps_exponent(po["REB_EPS"][i], init[i][0]), bc.eps_exponent(px["REB_EPS"][i], init[i][0])), (tag, "REB_EPS", i)
    report = pc.compare_solve(so, sx, len(phases), rtol=QUALIFY * 1e-6, atol_K=QUALIFY * 1e-6, tag=tag)
    print(f"[barrier] qualify {tag}: oracle-vs-long-double / (0.05 x tolerance) {bc.worst_ratio(report)}, n_iters {io['n_iters'].tolist()}, "
          f"n_ls_iters {io['n_ls_iters'].tolist()}")


@pytest.mark.parametrize("n_al", bc.AL_ITERS)
@pytest.mark.parametrize("name", bc.UPDATE_CASES)
def test_update_inputs_qualify(update_solves, name, n_al):
    phases, x0, so, sx = update_solves(name, n_al)
    _builds_agree(f"{name} max_AL_iter {n_al}", phases, x0, so, sx)


def test_window_shift_qualifies(oracle_lib, oracle_ld_lib):
    """wb_updates, max_AL_iter 2, then the window one knot later and a second solve - on fresh handles, the cached ones stay as they are.  The
    oracle's reconfigure moves the parameters as barrier_common.expected_after_shift states."""
    phases, x0, option = bc.update_case("wb_updates")
    so, sx = bc.make(oracle_lib, phases, x0), bc.make(oracle_ld_lib, phases, x0)
    try:
        so.solve(option(2)); sx.solve(option(2))
        before = bc.params(so)
        new = bc.shift_window(so); bc.shift_window(sx)
        want, got = bc.expected_after_shift(before, new, x0.shape[0]), bc.params(so)
        for f in bc.PARAM_FIELDS:
            for i in range(len(new)):
                assert np.array_equal(got[f][i], want[f][i]), (f, i)
        moved = [i for i, src in enumerate(bc.WB_SHIFT_SRC) if src >= 0 and not np.array_equal(got["REB_DELTA"][i], bc.initial_params(new, x0.shape[0])[i][1])]
        assert len(moved) == 3, moved      # every surviving phase carries updated entries: a copy of the initial values would show
        so.solve(option(2)); sx.solve(option(2))
        _builds_agree("wb_updates after the window shift", new, x0, so, sx, from_initial=False)
    finally:
        so.close(); sx.close()


@pytest.mark.parametrize("name", bc.UPDATE_CASES)
def test_update_coverage(update_solves, name):
    """Every barrier group of the model has entries that were updated and entries that were not; delta is seen strictly between its start and its
    floor and clamped to the floor; the floors reached differ pairwise across groups; eps and delta of an entry moved together.  Whole body:
    AL_SIGMA shows an uncapped product, the cap and an untouched value, AL_LAMBDA a changed and an unchanged entry.  Kinodynamic: every touchdown
    stays above 0.005, so sigma shows the product and the cap only.  The single-rigid-body tail has no terminal constraint."""
    phases, x0 = update_solves(name, 1)[:2]
    init = bc.initial_params(phases, x0.shape[0])
    groups = sorted({g for p in phases for _, _, g in bc.layout(p["desc"])})
    assert groups == dict(wb_updates=["grf", "joint", "jointspeed", "minheight", "torque"], hkd_updates=["grf"], srb_updates=["minheight"])[name]
    reb = {g: bc.group_params(next(p["desc"] for p in phases if any(x[2] == g for x in bc.layout(p["desc"]))), g) for g in groups}
    assert len({(r.delta, r.delta_min, r.eps) for r in reb.values()}) == len(groups)
    assert any(np.log2(r.delta / r.delta_min) % 1 != 0 for r in reb.values())        # some floor clamps to a value the halving alone does not reach
    updated, kept, between, clamped, floors = {}, {}, {}, {}, {}
    sigmas, lam_changed, lam_kept = set(), False, False
    for n_al in bc.AL_ITERS:
        so = update_solves(name, n_al)[2]
        par = bc.params(so)
        for i, p in enumerate(phases):
            eps, delta = par["REB_EPS"][i], par["REB_DELTA"][i]
            e0, d0, fl = init[i]
            ex = bc.eps_exponent(eps, e0)
            assert ex.min() >= 0 and ex.max() <= n_al, (name, n_al, i)
            assert np.array_equal(delta, np.maximum(d0 * bc.UPDATE_RELAX ** ex, fl)), (name, n_al, i)
            for c, (_, _, g) in enumerate(bc.layout(p["desc"])):
                col, dcol = ex[:, :, c], delta[:, :, c]
                updated[g] = updated.get(g, 0) + int((col > 0).sum()); kept[g] = kept.get(g, 0) + int((col == 0).sum())
                between[g] = between.get(g, 0) + int(((dcol < d0[:, :, c]) & (dcol > fl[:, :, c])).sum())
                at_floor = dcol == fl[:, :, c]
                clamped[g] = clamped.get(g, 0) + int(at_floor.sum())
                if at_floor.any():
                    floors[g] = float(fl[0, 0, c])
            sigmas |= set(np.unique(par["AL_SIGMA"][i]).tolist())
            lam = par["AL_LAMBDA"][i]
            lam_changed |= bool((lam != p["desc"].al_td.lambda_).any()); lam_kept |= bool((lam == p["desc"].al_td.lambda_).any())
    print(f"[barrier] updates {name}: entries over max_AL_iter 1-4: updated {updated}, not updated {kept}, delta between start and floor {between}, "
          f"at the floor {clamped}; floors {floors}; sigma values {sorted(sigmas)}")
    for g in groups:
        assert updated[g] > 0 and kept[g] > 0, (g, updated, kept)
        assert between[g] > 0 and clamped[g] > 0, (g, between, clamped)
    assert len(set(floors.values())) == len(groups) == len(floors), floors
    if name != "srb_updates":
        al = next(p["desc"].al_td for p in phases if p["desc"].c_touchdown)
        product = al.sigma * 5.0
        assert product < al.sigma_max < product * 5.0
        assert product in sigmas and al.sigma_max in sigmas, sigmas
    if name == "wb_updates":
        assert al.sigma in sigmas, sigmas
        assert lam_changed and lam_kept
