"""One process per GPU: rank start-up, ensemble sharding and the single collective of the multi-GPU path.

The HS-DDP path shards by independent problems: rank r owns a contiguous block of the ensemble, solves it with its own handle and no
data-path collective; one all-gather of the 64-byte per-problem result struct (RCCL over xGMI; `nccl` IS RCCL on ROCm) puts every
problem's outcome on every rank (arg-min over contact-schedule candidates, MHPCLocomotion-style consumers).  bench.py and the CPU
rehearsal in tests/test_sharding_gloo.py (gloo) go through the same functions.
"""
import os
import socket
import subprocess
import sys

import numpy as np

RESULT_FIELDS = ("actual_cost", "dyn_feas", "max_tconstr", "max_pconstr", "n_iters", "n_ls_iters", "n_reg_iters", "status")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def count_gpus_without_hip():
    """GPUs this process may use, counted WITHOUT touching the HIP runtime (the parent of the ranks must not initialise the GPU): KFD topology
    nodes with SIMDs under /sys/class/kfd, cut down by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES.  None when the topology is not readable
    (no amdgpu driver on this host): the ranks then find out themselves and fail loudly."""
    root = "/sys/class/kfd/kfd/topology/nodes"
    if not os.path.isdir(root):
        return None
    n = 0
    for node in sorted(os.listdir(root)):
        try:
            props = dict(line.split(None, 1) for line in open(os.path.join(root, node, "properties")).read().splitlines() if " " in line)
        except OSError:        # (a node of another container's cgroup: not ours)
            continue
        if int(props.get("simd_count", "0")) > 0:
            n += 1
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


def maybe_spawn(n_ranks, script, argv, require_gpus=True):
    """Parent side of `bench.py --gpus N` started WITHOUT a launcher: start N ranks (torch.distributed.run, one per GPU) as child
    processes and relay their output.  Must run before this process makes any GPU call (a process that has initialised the GPU must
    not exec or fork GPU work).  Returns None when this process is itself a rank (or N == 1), else the children's exit code."""
    if "WORLD_SIZE" in os.environ:
        if int(os.environ["WORLD_SIZE"]) != n_ranks:
            print(f"[launch] --gpus {n_ranks} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks", file=sys.stderr)
            raise SystemExit(2)
        return None
    if n_ranks <= 1:
        return None
    if require_gpus:
        have = count_gpus_without_hip()
        if have is None:
            have = 0 if not os.path.exists("/dev/kfd") else None      # no amdgpu device node at all: certainly no GPU here
        if have is not None and have < n_ranks:
            print(f"[launch] --gpus {n_ranks} requested but this node exposes {have} GPU(s): refusing to run fewer ranks than asked", file=sys.stderr)
            return 3
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), script] + list(argv)
    # HSA_ENABLE_IPC_MODE_LEGACY: the pool's host driver only supports dmabuf IPC (RCCL otherwise fails with hipIpcGetMemHandle: invalid argument);
    # the image exports 0 already - an explicit setting of the caller is passed through untouched
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def init_ranks(backend):
    """(rank, world, local_rank, dist or None).  backend: "nccl" (RCCL, one GPU per rank) or "gloo" (CPU rehearsal)."""
    rank, world, local = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1 and os.environ.get("HSDDP_FORCE_PROCESS_GROUP", "0") != "1":
        return 0, 1, local, None      # (HSDDP_FORCE_PROCESS_GROUP=1: a one-rank group all the same - runs every RCCL call of the N > 1 path on a one-GPU box)
    import torch
    import torch.distributed as dist
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend=backend)
    seen = dist.get_world_size()
    if seen != world:
        raise RuntimeError(f"process group reports {seen} ranks, launcher announced {world}")
    return rank, world, local, dist


def shard(total, world, rank):
    """Contiguous block [first, first + count) of `total` problems owned by `rank` (blocks differ by at most one problem)."""
    base, rem = divmod(total, world)
    count = base + (1 if rank < rem else 0)
    first = rank * base + min(rank, rem)
    return first, count


def result_rows(info):
    """hsddp_info_t arrays -> [problems, 8] fp64 rows (the 64-byte result struct of SURVEY 8e)."""
    return np.stack([np.asarray(info[k], dtype=np.float64) for k in RESULT_FIELDS], axis=1)


def gather_results(dist, rows, device):
    """All-gather of the per-problem result rows (blocks may differ in length by one: padded to the longest, trimmed after)."""
    import torch
    if dist is None:
        return rows
    world = dist.get_world_size()
    n = torch.tensor([rows.shape[0]], device=device, dtype=torch.int64)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n)
    nmax = int(max(int(x.item()) for x in ns))
    pad = torch.zeros((nmax, rows.shape[1]), device=device, dtype=torch.float64)
    pad[:rows.shape[0]] = torch.as_tensor(rows, device=device)
    out = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(out, pad)
    return np.concatenate([o[:int(c.item())].cpu().numpy() for o, c in zip(out, ns)])


def max_over_ranks(dist, value, device):
    if dist is None:
        return value
    import torch
    t = torch.tensor([value], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(dist, value, device):
    if dist is None:
        return value
    import torch
    t = torch.tensor([value], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def gather_scalars(dist, values, device):
    """[world, len(values)] fp64: a few per-rank scalars (solve time, iteration count) on every rank - explains a scaling result by rank."""
    row = np.asarray(values, dtype=np.float64)[None]
    if dist is None:
        return row
    import torch
    t = torch.as_tensor(row, device=device)
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return np.concatenate([o.cpu().numpy() for o in out])


# --------------------------------------------------------------------------------------------- schedule-candidate ensembles
def shard_candidates(S, B, world, rank):
    """The rank's share of an S-candidate x B-state ensemble: shard() of the candidate-major grid of S*B (candidate, state) units, cut into
    per-candidate segments [(cand, first_state, count), ...] in grid order.  Ranks get equal work (within one unit) also when S < world, and
    every segment is one schedule: one handle of `count` states drawn from the x0 stream at `first_state`."""
    first, count = shard(S * B, world, rank)
    segs, u, end = [], first, first + count
    while u < end:
        c, s = divmod(u, B)
        n = min(B - s, end - u)
        segs.append((c, s, n)); u += n
    return segs


def tagged_rows(segs, rows):
    """Result rows of a rank's segments (concatenated in segment order) with the (cand, state) of every row appended: [n, 10]."""
    tags = np.concatenate([np.stack([np.full(n, c), np.arange(s, s + n)], axis=1) for c, s, n in segs]) if segs else np.zeros((0, 2))
    return np.hstack([np.asarray(rows, dtype=np.float64).reshape(-1, 8), tags.astype(np.float64)])


def ensemble_rows(gathered, S, B):
    """Gathered tagged rows -> [S, B, 8]; every (cand, state) exactly once."""
    out = np.full((S, B, 8), np.nan)
    seen = np.zeros((S, B), dtype=np.int64)
    c, s = gathered[:, 8].astype(np.int64), gathered[:, 9].astype(np.int64)
    out[c, s] = gathered[:, :8]
    np.add.at(seen, (c, s), 1)
    if not (seen == 1).all():
        raise RuntimeError("gathered ensemble rows do not cover every (candidate, state) exactly once")
    return out


def owned_winners(S, B, world, rank, winner):
    """The winners `rank` holds, in state order: [(state, segment index, problem inside the segment's handle), ...]."""
    out = []
    for i, (c, s, n) in enumerate(shard_candidates(S, B, world, rank)):
        out += [(st, i, st - s) for st in range(s, s + n) if int(winner[st]) == c]
    return sorted(out)


def gather_policies(dist, S, B, winner, pack, row_words, device):
    """Second gather of the ensemble path: every rank packs the winners it owns (pack(list of (segment, problem)) -> [k, row_words] int32
    torch tensor on `device`, or a numpy array of 32-bit words), one padded all-gather, reassembled to [B, row_words] uint32 in state
    order.  The per-rank counts follow from the winners every rank already has: no size exchange."""
    import torch
    world = 1 if dist is None else dist.get_world_size()
    rank = 0 if dist is None else dist.get_rank()
    owned = [owned_winners(S, B, world, r, winner) for r in range(world)]
    mine = owned[rank]
    rows = pack([(i, p) for _, i, p in mine])
    rows = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rows).view(np.int32))
    rows = rows.to(device)
    assert tuple(rows.shape) == (len(mine), row_words)
    out = np.zeros((B, row_words), dtype=np.uint32)
    if dist is None:
        out[[st for st, _, _ in mine]] = rows.cpu().numpy().view(np.uint32)
        return out
    nmax = max(len(o) for o in owned)
    pad = torch.zeros((max(nmax, 1), row_words), dtype=torch.int32, device=device)
    pad[:len(mine)] = rows
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    for o, p in zip(owned, parts):
        if o:
            out[[st for st, _, _ in o]] = p[:len(o)].cpu().numpy().view(np.uint32)
    return out
