"""CPU tests of the schedule-candidate ensemble layer (include/hsddp_ensemble.h): its symbols, the selection rule (numpy specification
ensemble.select_rows against the device rule of csrc/ensemble.hpp compiled for the host), and the candidate-major sharding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT

CSRC = os.path.join(ROOT, "cafe-mpc_amd", "csrc")


def test_ensemble_header_symbols_match_binding_list():
    hdr = open(os.path.join(ROOT, "include", "hsddp_ensemble.h")).read()
    assert sorted(set(re.findall(r"\b(hsddp_[a-zA-Z_]+)\s*\(", hdr))) == sorted(pkg._abi.ENSEMBLE_EXPORTS)
    assert not set(pkg._abi.ENSEMBLE_EXPORTS) & set(pkg._abi.EXPORTS)


def test_fresh_hip_build_exports_the_ensemble_symbols(tmp_path):
    """A fresh hipcc --offload-arch=gfx950 build of libhsddp_hip.so (the product Makefile's recipe, into a scratch directory)."""
    so = tmp_path / "libhsddp_hip.so"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           "-Wno-unused-value", "-DROLL_WPE=2", os.path.join(CSRC, "hsddp_hip.hip"), "-o", str(so)], timeout=1800)
    lib = ctypes.CDLL(str(so))
    for s in pkg._abi.ENSEMBLE_EXPORTS + pkg._abi.EXPORTS:
        assert hasattr(lib, s), s
    pkg._abi.bind_ensemble(lib)


def test_bind_ensemble_refuses_a_library_without_it(oracle_lib):
    with pytest.raises(RuntimeError):
        pkg._abi.bind_ensemble(oracle_lib)


DRIVER = r"""
#include <cstdio>
#include <vector>
#include "ensemble.hpp"
// stdin: S B td tt tp, then S*B rows of 8 doubles (candidate-major); stdout: B winners
int main() {
    int S, B; double td, tt, tp;
    if (scanf("%d %d %lf %lf %lf", &S, &B, &td, &tt, &tp) != 5) return 1;
    std::vector<double> r((size_t)S * B * 8);
    for (auto& v : r) { unsigned long long u; if (scanf("%llx", &u) != 1) return 2; __builtin_memcpy(&v, &u, 8); }
    for (int b = 0; b < B; b++) {
        int w = 0; hs::EnsRank best;
        for (int c = 0; c < S; c++) {
            const double* x = &r[((size_t)c * B + b) * 8];
            hs::EnsRank k = hs::ens_rank(x[0], x[1], x[2], x[3], (int)x[7], td, tt, tp);
            if (c == 0 || hs::ens_better(k, best)) { best = k; w = c; }
        }
        printf("%d\n", w);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def device_rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("rule")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DENS_RULE_ONLY", "-I", CSRC, str(d / "drv.cpp"), "-o", str(exe)])

    def run(rows, opt):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        S, B = rows.shape[:2]
        txt = f"{S} {B} {opt.dynamics_feas_thresh!r} {opt.tconstr_thresh!r} {opt.pconstr_thresh!r}\n" + " ".join(f"{u:x}" for u in rows.reshape(-1).view(np.uint64))
        out = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, check=True).stdout
        return np.array([int(x) for x in out.split()], dtype=np.int32)
    return run


def _row(cost, dyn=0.0, tc=0.0, pc=0.0, status=0):
    return [cost, dyn, tc, pc, 3, 4, 0, status]


OPT = pkg.mhpc_ddp_setting()      # thresholds 1e-3 each


CASES = {
    # name: (candidates' rows for ONE state, expected winner)
    "cheapest_admissible": ([_row(5.0), _row(3.0), _row(4.0)], 1),
    "tie_goes_to_lowest_index": ([_row(4.0), _row(3.0), _row(3.0)], 1),
    "all_equal": ([_row(1.0)] * 4, 0),
    "nan_cost_is_tier2": ([_row(np.nan), _row(9.0)], 1),
    "nan_feas_is_tier2": ([_row(1.0, dyn=np.nan), _row(9.0)], 1),
    "status1_is_tier2": ([_row(1.0, status=1), _row(9.0)], 1),
    "status2_is_admissible": ([_row(9.0), _row(1.0, status=2)], 1),
    "violation_exactly_at_threshold_is_tier0": ([_row(9.0, dyn=2e-3), _row(5.0, pc=1e-3)], 1),
    "just_above_threshold_is_tier1": ([_row(1.0, tc=np.nextafter(1e-3, 1.0)), _row(5.0)], 1),
    "tier1_by_violation_then_cost": ([_row(1.0, dyn=5e-3), _row(7.0, pc=2e-3), _row(6.0, tc=2e-3)], 2),
    "all_inadmissible_first_wins": ([_row(1.0, status=1), _row(np.nan), _row(2.0, status=1)], 0),
    "single_candidate": ([_row(np.nan, status=1)], 0),
    "inf_cost": ([_row(np.inf), _row(1e300)], 1),
    "negative_zero_ties": ([_row(0.0), _row(-0.0)], 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_rule_crafted(name, device_rule):
    cands, want = CASES[name]
    rows = np.array(cands, dtype=np.float64)[:, None, :]          # [S, 1, 8]
    spec = pkg.ensemble.select_rows(rows, OPT)
    assert spec[0] == want, (name, spec)
    assert np.array_equal(device_rule(rows, OPT), spec)


def test_selection_rule_random_agrees_bitwise(device_rule):
    """Many states at once, values drawn around the thresholds, with NaNs, statuses and exact ties mixed in."""
    rng = np.random.default_rng(7)
    S, B = 5, 2000
    rows = np.zeros((S, B, 8))
    rows[..., 0] = rng.choice([1.0, 2.0, 3.0, np.nan, np.inf], size=(S, B), p=[0.3, 0.3, 0.3, 0.05, 0.05]) + rng.integers(0, 2, (S, B)) * rng.random((S, B))
    for f in (1, 2, 3):
        rows[..., f] = rng.choice([0.0, 1e-3, 5e-4, 2e-3, np.nan], size=(S, B), p=[0.4, 0.2, 0.2, 0.15, 0.05])
    rows[..., 7] = rng.choice([0, 1, 2], size=(S, B), p=[0.7, 0.15, 0.15])
    for opt in (OPT, pkg.mhpc_ddp_setting(dynamics_feas_thresh=1e-2, tconstr_thresh=5e-4, pconstr_thresh=0.0)):
        spec = pkg.ensemble.select_rows(rows, opt)
        assert np.array_equal(device_rule(rows, opt), spec)
    assert len(set(spec.tolist())) == S


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("S", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_shard_candidates_owns_every_unit_once_in_order(world, S, B):
    units, work = [], []
    for r in range(world):
        segs = pkg.launch.shard_candidates(S, B, world, r)
        n = 0
        for c, s, cnt in segs:
            assert 0 <= c < S and 0 <= s and cnt >= 1 and s + cnt <= B
            units += [(c, st) for st in range(s, s + cnt)]; n += cnt
        assert len({c for c, _, _ in segs}) == len(segs)      # one segment (one handle) per schedule
        work.append(n)
    assert units == [(c, st) for c in range(S) for st in range(B)]
    assert max(work) - min(work) <= 1


def test_ensemble_rows_and_owned_winners_roundtrip():
    S, B, world = 3, 5, 2
    rows = np.arange(S * B * 8, dtype=np.float64).reshape(S, B, 8)
    parts = []
    for r in range(world):
        segs = pkg.launch.shard_candidates(S, B, world, r)
        parts.append(pkg.launch.tagged_rows(segs, np.concatenate([rows[c, s:s + n] for c, s, n in segs])))
    assert np.array_equal(pkg.launch.ensemble_rows(np.concatenate(parts[::-1]), S, B), rows)
    winner = np.array([2, 0, 1, 1, 2])
    owned = [pkg.launch.owned_winners(S, B, world, r, winner) for r in range(world)]
    assert sorted(st for o in owned for st, _, _ in o) == list(range(B))


def test_timing_candidates_share_the_horizon():
    for total in (200, 13, 16):
        c = pkg.problems.wb_trot_timing_candidates(total)
        assert len(c) == 4
        assert {sum(p["desc"].horizon for p in ph) for ph in c} == {total}
    assert [tuple(p["desc"].horizon for p in ph) for ph in pkg.problems.wb_trot_timing_candidates()] == list(pkg.problems.TROT_TIMINGS)
