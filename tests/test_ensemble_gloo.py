"""CPU rehearsal of the sharded schedule-candidate ensemble (world 2, gloo) through the launcher code tools/ensemble_bench.py uses: the
candidate-major grid of S x B (candidate, state) units split by launch.shard_candidates (uneven: 8 + 7 units, one candidate cut between
the ranks), one all-gather of the tagged result rows, select_rows on every rank, one padded all-gather of the winners' policies.  The
oracle library stands in for the solver (no GPU here; the rehearsal packs per problem with export_mpc_command); gathered rows, winners and
policy words must equal a one-process unsharded run bit for bit."""
import os
import subprocess
import sys
import textwrap

import numpy as np

from conftest import pkg, ROOT

S, B, TOTAL, SEED = 3, 5, 13, 99

WORKER = textwrap.dedent("""
    import ctypes, os, sys
    import numpy as np
    sys.path.insert(0, sys.argv[1])
    import __graft_entry__ as ge
    pkg = ge.load_package()
    launch = pkg.launch
    S, B, TOTAL, SEED = (int(x) for x in sys.argv[3:7])
    rc = launch.maybe_spawn(2, os.path.abspath(__file__), sys.argv[1:], require_gpus=False)
    if rc is not None:
        sys.exit(rc)
    rank, world, local, dist = launch.init_ranks("gloo")
    lib = pkg._abi.bind(ctypes.CDLL(os.path.join(sys.argv[1], "oracle", "liboracle_hsddp.so")))
    cands = pkg.problems.wb_trot_timing_candidates(TOTAL)[:S]
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2, cost_thresh=0.0)
    segs = launch.shard_candidates(S, B, world, rank)
    solvers = []
    for c, first, n in segs:
        s = pkg.Solver(lib, cands[c], batch=n)
        for i, p in enumerate(cands[c]):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(n, SEED, first=first))
        s.solve(opt)
        solvers.append(s)
    rows = np.concatenate([launch.result_rows(s.info_arrays()) for s in solvers])
    all_rows = launch.ensemble_rows(launch.gather_results(dist, launch.tagged_rows(segs, rows), "cpu"), S, B)
    winner = pkg.select_rows(all_rows, opt)
    W = pkg.ensemble.command_row_words(8)
    pack = lambda pairs: np.array([solvers[i].export_mpc_command(p, 8, 0.2, 0.01)["raw"] for i, p in pairs], dtype=np.uint32).reshape(-1, W)
    policies = launch.gather_policies(dist, S, B, winner, pack, W, "cpu")
    if rank == 0:
        np.savez(sys.argv[2], rows=all_rows, winner=winner, policies=policies)
    dist.barrier(); dist.destroy_process_group()
""")


def test_sharded_ensemble_equals_unsharded(oracle_lib, tmp_path):
    assert [sum(n for _, _, n in pkg.launch.shard_candidates(S, B, 2, r)) for r in range(2)] == [8, 7]
    w = tmp_path / "worker.py"; w.write_text(WORKER)
    out = tmp_path / "gathered.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "1"
    subprocess.check_call([sys.executable, str(w), ROOT, str(out), str(S), str(B), str(TOTAL), str(SEED)], env=env, timeout=900)
    got = np.load(out)
    cands = pkg.problems.wb_trot_timing_candidates(TOTAL)[:S]
    opt = pkg.mhpc_ddp_setting(max_AL_iter=1, max_DDP_iter=2, cost_thresh=0.0)
    solvers, rows = [], []
    for ph in cands:
        s = pkg.Solver(oracle_lib, ph, batch=B)
        for i, p in enumerate(ph):
            s.set_nominal(i, p["Xbar"], p["Ubar"])
        s.set_initial_condition(pkg.problems.wb_ensemble_x0(B, SEED))
        s.solve(opt)
        solvers.append(s); rows.append(pkg.launch.result_rows(s.info_arrays()))
    rows = np.stack(rows)
    winner = pkg.select_rows(rows, opt)
    policies = np.stack([solvers[int(winner[b])].export_mpc_command(b, 8, 0.2, 0.01)["raw"] for b in range(B)])
    assert np.array_equal(got["rows"], rows)
    assert np.array_equal(got["winner"], winner)
    assert np.array_equal(got["policies"], policies)
