"""Schedule-candidate ensembles on the MI355X (include/hsddp_ensemble.h, csrc/ensemble.hpp): parity of the concurrently solved candidates
with the CPU oracle, concurrency that changes no bit, k_ens_select against ensemble.select_rows, k_ens_pack rows against the per-handle
export, argument checks, the warm tick's zero allocations, and the one-rank RCCL run of tools/ensemble_bench.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg, ROOT

# The candidate set of the parity test: the four trot timings of problems.wb_trot_timing_candidates(200) over the states
# wb_ensemble_x0(64, 20241220), 1 AL x 2 DDP iterations.  Chosen on the CPU with the oracle: already the first 16 of these states split
# their winners between timing 0 (50/50/50/50) and timing 1 (40/60/40/60), so the arg-min is exercised (asserted below).
B, SEED = 64, 20241220


def parity_opt():
    return pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)


def wb_phases(ph):
    return [i for i, p in enumerate(ph) if p["desc"].model == pkg.MODEL_WB]


@pytest.fixture(scope="module")
def cands():
    return pkg.problems.wb_trot_timing_candidates(200)


@pytest.fixture(scope="module")
def hip_ens(cands):
    ens = pkg.ScheduleEnsemble(cands, B)
    ens.set_initial_condition(pkg.problems.wb_ensemble_x0(B, SEED))
    ens.solve(parity_opt(), concurrent=True)
    yield ens
    ens.close()


@pytest.fixture(scope="module")
def oracle_solvers(cands, oracle_lib):
    out = []
    for ph in cands:
        s = pkg.Solver(oracle_lib, ph, batch=B)
        for i, p in enumerate(ph):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(B, SEED))
        s.solve(parity_opt())
        out.append(s)
    return out


@pytest.mark.gpu
def test_parity_with_the_oracle(hip_ens, oracle_solvers, cands):
    opt = parity_opt()
    rows = hip_ens.rows()
    ref = np.stack([pkg.launch.result_rows(s.info_arrays()) for s in oracle_solvers])
    for f in (4, 5, 7):                                            # n_iters, n_ls_iters, status
        assert np.array_equal(rows[:, :, f], ref[:, :, f]), f
    assert np.allclose(rows[:, :, 0], ref[:, :, 0], rtol=1e-8, atol=0)
    w, _ = hip_ens.select(opt)
    wref = pkg.select_rows(ref, opt)
    assert np.array_equal(w, wref)
    assert len(set(w.tolist())) >= 2, np.bincount(w)
    for b in range(B):
        c = int(w[b])
        for i in wb_phases(cands[c]):
            dK = np.abs(hip_ens.solvers[c].field(i, "K", b, 1) - oracle_solvers[c].field(i, "K", b, 1)).max()
            assert dK < 1e-6, (b, c, i, dK)


@pytest.mark.gpu
def test_concurrency_is_invisible(hip_ens, cands):
    seq = pkg.ScheduleEnsemble(cands, B)
    seq.set_initial_condition(pkg.problems.wb_ensemble_x0(B, SEED))
    seq.solve(parity_opt(), concurrent=False)
    a, b = hip_ens.rows(), seq.rows()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for c, ph in enumerate(cands):
        for i in range(len(ph)):
            for f in ("K", "XBAR", "UBAR"):
                x, y = hip_ens.solvers[c].field(i, f), seq.solvers[c].field(i, f)
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (c, i, f)
    seq.close()


@pytest.mark.gpu
def test_device_selection_equals_the_spec(hip_ens):
    opt = parity_opt()
    w, best = hip_ens.select(opt)
    rows = hip_ens.rows()
    assert np.array_equal(w, pkg.select_rows(rows, opt))
    assert np.array_equal(best.view(np.uint64), rows[w, np.arange(B)].view(np.uint64))
    strict = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2, dynamics_feas_thresh=1.0, tconstr_thresh=1.0, pconstr_thresh=1.0)
    w2, _ = hip_ens.select(strict)                                 # other thresholds: other tiers, same agreement
    assert np.array_equal(w2, pkg.select_rows(rows, strict))


@pytest.mark.gpu
def test_export_rows_bit_equal_to_the_per_handle_export(hip_ens, cands):
    import ctypes as C
    rt = C.CDLL("libamdhip64.so.7")                                # the HIP runtime libhsddp_hip.so itself runs on (device destination)
    w, _ = hip_ens.select(parity_opt())
    rng = np.random.default_rng(3)
    pairs = [(int(w[b]), b) for b in range(B)] + [(int(c), int(b)) for c, b in zip(rng.integers(0, 4, 16), rng.integers(0, B, 16))]
    status = [np.arange(len(ph) * 4, dtype=np.float32).reshape(-1, 4) * (c + 1) * 0.01 for c, ph in enumerate(cands)]
    status[2] = None                                               # a candidate without status times: zeros
    n_steps = 8
    host = hip_ens.export_mpc_commands(pairs, n_steps, mpc_time=0.37, dt=0.01, status_times=status)
    p = C.c_void_p()
    assert rt.hipMalloc(C.byref(p), C.c_size_t(host.nbytes)) == 0
    try:
        hip_ens.export_mpc_commands(pairs, n_steps, mpc_time=0.37, dt=0.01, status_times=status, out=p.value)
        dev = np.zeros_like(host)
        assert rt.hipMemcpy(C.c_void_p(dev.ctypes.data), p, C.c_size_t(host.nbytes), 2) == 0       # hipMemcpyDeviceToHost
    finally:
        rt.hipFree(p)
    nost = hip_ens.export_mpc_commands(pairs[:4], n_steps, mpc_time=0.37, dt=0.01)
    for i, (c, b) in enumerate(pairs):
        ref = hip_ens.solvers[c].export_mpc_command(b, n_steps, 0.37, 0.01, status_times=status[c])["raw"]
        assert np.array_equal(host[i], ref), (i, c, b)
        assert np.array_equal(dev[i], ref), (i, c, b)
        if i < 4:
            assert np.array_equal(nost[i], hip_ens.solvers[c].export_mpc_command(b, n_steps, 0.37, 0.01)["raw"])
    # 60 knots: candidate 1 (40 knots in its first phase) crosses a phase boundary at another step than candidate 0 (50)
    long_ = hip_ens.export_mpc_commands([(0, 3), (1, 3), (2, 5)], 60, mpc_time=0.1, dt=0.01)
    for i, (c, b) in enumerate([(0, 3), (1, 3), (2, 5)]):
        assert np.array_equal(long_[i], hip_ens.solvers[c].export_mpc_command(b, 60, 0.1, 0.01)["raw"])


@pytest.mark.gpu
def test_export_refuses_knots_that_are_not_whole_body():
    ph = pkg.problems.mhpc_problem(wb_horizons=(2, 2))            # 4 whole-body control knots, then single-rigid-body phases
    ens = pkg.ScheduleEnsemble([ph], 1)
    ens.export_mpc_commands([(0, 0)], 4)
    with pytest.raises(RuntimeError, match="rc=-1"):
        ens.export_mpc_commands([(0, 0)], 8)
    with pytest.raises(RuntimeError, match="rc=-1"):
        ens.export_mpc_commands([(0, 1)], 2)                       # problem out of range
    ens.close()


@pytest.mark.gpu
def test_create_rejects_mismatched_candidates(hip_lib):
    import ctypes as C
    lib = pkg._abi.bind_ensemble(hip_lib)
    a = pkg.MultiPhaseDDP(pkg.problems.wb_trot_problem(horizons=(4, 4, 4, 4)), batch=1)
    b = pkg.MultiPhaseDDP(pkg.problems.wb_trot_problem(horizons=(4, 4, 4, 5)), batch=1)          # horizon time 0.17 s vs 0.16 s
    c = pkg.MultiPhaseDDP(pkg.problems.hkd_trot_problem(horizons=(4, 4, 4, 4)), batch=1)         # phase 0: 24 states vs 36
    d = pkg.MultiPhaseDDP(pkg.problems.wb_trot_problem(horizons=(3, 5, 3, 5)), batch=2)          # same horizon time, other batch: accepted
    e = C.c_void_p()
    for pair, rc in (((a, b), -1), ((a, c), -1), ((a, d), 0)):
        hs = (C.c_void_p * 2)(pair[0].h.value, pair[1].h.value)
        assert lib.hsddp_ensemble_create(C.byref(e), 2, hs) == rc
        if rc == 0:
            w = np.zeros(2, dtype=np.int32)
            assert lib.hsddp_ensemble_select(e, C.byref(parity_opt()), w.ctypes.data_as(pkg._abi.IP), None) == -1      # batches differ
            lib.hsddp_ensemble_destroy(e)
    import torch
    if torch.cuda.device_count() > 1:                              # candidates on two devices
        f = pkg.MultiPhaseDDP(pkg.problems.wb_trot_problem(horizons=(4, 4, 4, 4)), batch=1, device=1)
        hs = (C.c_void_p * 2)(a.h.value, f.h.value)
        assert lib.hsddp_ensemble_create(C.byref(e), 2, hs) == -1


@pytest.mark.gpu
def test_warm_tick_makes_no_device_allocation(hip_lib, cands):
    ens = pkg.ScheduleEnsemble(cands, 1)
    ens.set_initial_condition(pkg.problems.wb_ensemble_x0(1, SEED))
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2)
    status = [np.zeros((len(ph), 4), dtype=np.float32) for ph in cands]
    counts = []
    for tick in range(3):            # the same tick three times (nominal and x0 reset): a handle's line-search staging grows with the deepest search it has met
        for s, ph in zip(ens.solvers, cands):
            for i, p in enumerate(ph):
                s.set_nominal(i, p["Xbar"], p["Ubar"])
        ens.set_initial_condition(pkg.problems.wb_ensemble_x0(1, SEED))
        ens.solve(opt, max_cputime_ms=1e6, concurrent=True)
        w, _ = ens.select(opt)
        ens.export_mpc_commands([(int(w[0]), 0)], 8, mpc_time=0.01 * tick, status_times=status)
        counts.append(hip_lib.hsddp_debug_malloc_count())
    assert counts[0] == counts[1] == counts[2], counts
    ens.close()


@pytest.mark.gpu
def test_rccl_calls_of_the_ensemble_bench_on_one_rank(tmp_path, cands):
    """tools/ensemble_bench.py --gpus 1 under torch.distributed.run in a ONE-rank RCCL group (HSDDP_FORCE_PROCESS_GROUP=1): both all-gathers
    (tagged rows, winners' policies) run; what they gather equals the unsharded ensemble of this process."""
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    dump = tmp_path / "dist.npz"
    env = dict(os.environ, HSDDP_FORCE_PROCESS_GROUP="1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tools", "ensemble_bench.py"), "--gpus", "1", "--dist-only", "--dist-batch", "8", "--total", "40", "--tick-iters", "2",
           "--dump", str(dump)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["collectives"] == "rccl" and line["n_gpus"] == 1
    d = np.load(dump)
    small = pkg.problems.wb_trot_timing_candidates(40)
    ens = pkg.ScheduleEnsemble(small, 8)
    ens.set_initial_condition(pkg.problems.wb_ensemble_x0(8, SEED))
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2, cost_thresh=0.0)
    ens.solve(opt)
    rows = ens.rows()
    w, _ = ens.select(opt)
    assert np.array_equal(d["rows"].view(np.uint64), rows.view(np.uint64))
    assert np.array_equal(d["winner"], w)
    assert np.array_equal(d["policies"], ens.export_mpc_commands([(int(w[b]), b) for b in range(8)], 8))
    ens.close()
