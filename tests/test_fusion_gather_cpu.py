"""world_size-2 gloo test (CPU) of parallel_rollout.gather_fusion: the fused cloud's raw sums and counts travel in one float64
all_gather of their own, and rank 0 forms the ratios."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

THRESHOLDS, CAP = (0.5, 1.0), 5.0
OPTIONS = {"voxel": 0.25, "trunc": 1.0, "min_weight": 1, "max_depth": 70.0}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raw(rid):
    """Run rid's raw vector: counts beyond 2^24 and sums that fp32 would not carry."""
    from nextbestpath_amd.utility import recon_metrics as rm
    from nextbestpath_amd.utility import tsdf
    rng = np.random.default_rng(rid)
    n_rec, n_gt = 20_000_000 + rid, 30_000_001 + 7 * rid
    row = rm.pack_raw(rng.uniform(0, 1e6, 2) + 1e-9, rng.integers(0, n_rec, 2), n_rec, rng.uniform(0, 1e6, 2) + 1e-9,
                      rng.integers(0, n_gt, 2), n_gt)
    return tsdf.pack_raw(row, 2 ** 27 + rid, 2 ** 25 + 3 * rid, 505 - rid)


def _worker(rank, world, port, n_runs, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    runs = [(i, 0) for i in range(n_runs)]
    results = [{"run_id": runs.index(run), "fusion_raw": _raw(runs.index(run)).tolist()} for run in reversed(pr.shard(runs, r, w))]
    q.put((r, pr.gather_fusion(results, runs, r, w, torch.device("cpu"), THRESHOLDS, CAP, OPTIONS)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gather_fusion_world2():
    from nextbestpath_amd.utility import tsdf
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
        assert block == tsdf.summarise_raw(_raw(rid), THRESHOLDS, CAP, OPTIONS)      # float64 all the way: equal, not close
        assert block["n_points"] == 20_000_000 + rid and block["observed_voxels"] == 2 ** 27 + rid and block["frames"] == 505 - rid
        assert block["options"] == OPTIONS and len(block["thresholds"]) == 2


def test_gather_fusion_single_process():
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.utility import tsdf
    res = [{"run_id": i, "fusion_raw": _raw(i).tolist()} for i in range(2)]
    out = pr.gather_fusion(res, [(0, 0), (1, 0)], 0, 1, torch.device("cpu"), THRESHOLDS, CAP, OPTIONS)
    assert out == {i: tsdf.summarise_raw(_raw(i), THRESHOLDS, CAP, OPTIONS) for i in range(2)}
    assert out[0]["options"] is not OPTIONS and "options" not in pr.gather_fusion(res[:1], [(0, 0)], 0, 1, torch.device("cpu"), THRESHOLDS,
                                                                                   CAP)[0]
