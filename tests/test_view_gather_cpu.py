"""world_size-2 gloo test (CPU) of parallel_rollout.gather_views: the held-out view metrics' raw rows travel in one float64
all_gather of their own, and rank 0 forms the ratios."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

OPTIONS = {"views": 4, "seed": 0, "radius": 1, "depth_tolerance": 1.0, "height": 24, "width": 40, "z_far": 50.0}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raw(rid):
    """Run rid's raw rows: rid % 4 + 1 views (run 3 has the option's 4, the others fewer), counts beyond 2^24 and sums that fp32
    would not carry."""
    rng = np.random.default_rng(rid)
    n = rid % 4 + 1
    rows = np.zeros((n, 9))
    rows[:, 0] = 20_000_000 + rng.integers(0, 1000, n)           # n_gt
    rows[:, 2] = rng.integers(1, 10_000_000, n)                  # n_hit
    rows[:, 1] = rows[:, 2] + rng.integers(0, 1000, n)           # n_c
    rows[:, 3:6] = rng.integers(0, 1000, (n, 3))
    rows[:, 6:9] = rng.uniform(0, 1e6, (n, 3)) + 1e-9
    return rows


def _worker(rank, world, port, n_runs, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    runs = [(i, 0) for i in range(n_runs)]
    results = [{"run_id": runs.index(run), "views_raw": _raw(runs.index(run)).tolist()} for run in reversed(pr.shard(runs, r, w))]
    q.put((r, pr.gather_views(results, runs, r, w, torch.device("cpu"), OPTIONS)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gather_views_world2():
    from nextbestpath_amd.utility import view_metrics as vm
    n_runs, world = 5, 2                       # odd count: rank 1 has a padded row
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_runs, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[1] == {}                        # the ratios are formed on rank 0 alone
    assert sorted(got[0]) == list(range(n_runs))
    for rid, block in got[0].items():
        assert block == vm.summarise_raw(_raw(rid), OPTIONS)             # float64 all the way: equal, not close
        assert block["n_views"] == rid % 4 + 1 and block["options"] == OPTIONS and block["n_gt"] > 2 ** 24


def test_gather_views_single_process_and_too_many_views():
    import pytest
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.utility import view_metrics as vm
    res = [{"run_id": i, "views_raw": _raw(i).tolist()} for i in range(2)]
    out = pr.gather_views(res, [(0, 0), (1, 0)], 0, 1, torch.device("cpu"), OPTIONS)
    assert out == {i: vm.summarise_raw(_raw(i), OPTIONS) for i in range(2)}
    with pytest.raises(ValueError):
        pr.gather_views([{"run_id": 0, "views_raw": np.zeros((5, 9)).tolist()}], [(0, 0)], 0, 1, torch.device("cpu"), OPTIONS)
