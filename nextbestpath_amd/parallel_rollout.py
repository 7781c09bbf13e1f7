"""Scene-parallel sharding of independent rollouts.

Each (scene, start pose) rollout is independent (next_best_path/testers/nbp_planning.py:414-467
runs them in nested loops on one GPU), so rank r takes runs r, r+W, r+2W, ... and the only
collective is ONE all_gather of a padded fp32 tensor [runs_per_rank, n_poses + 3] holding
(run id, final coverage, AUC, coverage curve) -- a few KB over RCCL/xGMI, latency bound (with the
planning option `recon_metrics` on, a second one of float64 sums and counts: gather_reconstruction; with its `curve`, a third of the
per-step rows: gather_reconstruction_curve; with the option `view_metrics`, one of the per-view counts and sums: gather_views; with the option `fusion`, one of the fused cloud's sums and counts: gather_fusion; with the option `surface_metrics`, one of both
clouds' sums and counts against the mesh: gather_surface).  One
process per GPU; backend "nccl" (= RCCL on ROCm) with CUDA tensors, "gloo" on CPU-only hosts
(that path is what the world_size-2 CPU tests exercise)."""
from __future__ import annotations

import os

import numpy as np
import torch


def init_distributed():
    """(rank, world, local_rank); initialises torch.distributed when launched under torchrun -- also with ONE rank
    (`torchrun --nproc-per-node 1`): the collectives then run through RCCL on the single GPU, which is how the `nccl`
    path is exercised on a 1-GPU box (tests/test_gpu_rccl.py)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 or under_torchrun():
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("NBP_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
            if backend == "nccl":
                torch.cuda.set_device(local_rank)
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            else:       # gloo: CPU-only hosts, or several ranks sharing one GPU (NBP_DIST_BACKEND=gloo) in tests
                dist.init_process_group("gloo")
            if rank == 0 and os.environ.get("NBP_TRACE_DIST"):
                print(f"[dist] backend {dist.get_backend()} world {dist.get_world_size()}", flush=True)
    if torch.cuda.is_available():
        local_rank = local_rank % torch.cuda.device_count()
    return rank, world, local_rank


def under_torchrun():
    return all(k in os.environ for k in ("WORLD_SIZE", "RANK", "MASTER_ADDR", "MASTER_PORT"))


def group_is_up():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def collective_device(device):
    """Tensors of the gather live on the GPU for RCCL and on the host for gloo."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == "gloo":
        return torch.device("cpu")
    return device


def shard(runs, rank, world):
    return list(runs)[rank::world]


def runs_per_rank(n_runs, world):
    return (n_runs + world - 1) // world


def pack_results(results, runs, n_poses, rows):
    """Local results -> padded [rows, n_poses + 3] fp32 (run id, final coverage, AUC, curve); pad rows = -1."""
    from .utility.long_term_utils import compute_auc
    t = np.full((rows, n_poses + 3), -1.0, np.float32)
    for j, r in enumerate(results):
        cov = np.asarray(r["coverage"], np.float32)
        t[j, 0] = r["run_id"]
        t[j, 1] = cov[-1]
        t[j, 2] = compute_auc(cov)
        t[j, 3:3 + len(cov)] = cov
    return t


def gather_results(results, runs, rank, world, device, n_poses):
    """All ranks call this; every rank gets the list of {run_id, coverage, final, auc, scene, start}
    in run order (only the coverage metrics travel; pose histories stay in the per-rank results)."""
    rows = runs_per_rank(len(runs), world)
    collective = world > 1 or group_is_up()          # a 1-rank process group still goes through the backend
    local = torch.from_numpy(pack_results(results, runs, n_poses, rows)).to(collective_device(device) if collective else device)
    if collective:
        import torch.distributed as dist
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        allt = torch.stack(buf).cpu().numpy().reshape(-1, n_poses + 3)
    else:
        allt = local.cpu().numpy()
    by_id = {int(r["run_id"]): r for r in results}
    out = []
    for row in allt:
        if row[0] < 0:
            continue
        rid = int(row[0])
        rec = dict(by_id[rid]) if rid in by_id else {}
        rec.update(run_id=rid, coverage=[float(v) for v in row[3:3 + n_poses]], final=float(row[1]), auc=float(row[2]))
        out.append(rec)
    out.sort(key=lambda r: r["run_id"])
    return out


def gather_reconstruction(results, runs, rank, world, device, thresholds, cap):
    """The planning option `recon_metrics`: all ranks call this behind gather_results.  The raw float64 sums and counts of every
    run's reconstruction metrics (results[i]["reconstruction_raw"], utility/recon_metrics.py::pack_raw) travel in ONE all_gather
    of a padded float64 tensor [runs_per_rank, 1 + 6 + 2 T] (run id first; pad rows = -1) -- a gather of its own, so that the
    coverage gather keeps its shape with the option off.  Rank 0 forms the ratios from them -> {run id: metrics dict}; the other
    ranks get {}."""
    from .utility import recon_metrics
    rows = runs_per_rank(len(runs), world)
    width = 1 + recon_metrics.RAW_HEAD + 2 * len(thresholds)
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        t[j, 0] = r["run_id"]
        t[j, 1:] = np.asarray(r["reconstruction_raw"], np.float64)
    collective = world > 1 or group_is_up()
    if collective:
        import torch.distributed as dist
        local = torch.from_numpy(t).to(collective_device(device))
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        t = torch.stack(buf).cpu().numpy().reshape(-1, width)
    if rank != 0:
        return {}
    return {int(row[0]): recon_metrics.summarise_raw(row[1:], thresholds, cap) for row in t if row[0] >= 0}


def gather_reconstruction_curve(results, runs, rank, world, device, thresholds, cap, n_poses):
    """The planning option `recon_metrics` with `curve`: all ranks call this behind gather_reconstruction.  The raw rows of every
    run's per-step curve (results[i]["reconstruction_curve_raw"]: n_poses rows of pack_raw's 6 + 2 T numbers) travel in ONE
    all_gather of a padded float64 tensor [runs_per_rank, 1 + n_poses (6 + 2 T)] (run id first; pad rows = -1) -- a gather of its
    own: the other two keep their shapes with the curve off.  Rank 0 forms the ratios -> {run id: summarise_curve's dict}; the
    other ranks get {}."""
    from .utility import recon_metrics
    rows = runs_per_rank(len(runs), world)
    per = recon_metrics.RAW_HEAD + 2 * len(thresholds)
    width = 1 + n_poses * per
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        t[j, 0] = r["run_id"]
        t[j, 1:] = np.asarray(r["reconstruction_curve_raw"], np.float64).reshape(n_poses * per)
    collective = world > 1 or group_is_up()
    if collective:
        import torch.distributed as dist
        local = torch.from_numpy(t).to(collective_device(device))
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        t = torch.stack(buf).cpu().numpy().reshape(-1, width)
    if rank != 0:
        return {}
    return {int(row[0]): recon_metrics.summarise_curve(row[1:].reshape(n_poses, per), thresholds, cap) for row in t if row[0] >= 0}


def gather_fusion(results, runs, rank, world, device, thresholds, cap, options=None):
    """The planning option `fusion`: all ranks call this behind gather_results, and only when the option is on.  The raw float64
    numbers of every run's fused cloud (results[i]["fusion_raw"], utility/tsdf.py::pack_raw: the reconstruction metrics' sums and
    counts, then observed_voxels, usable_voxels, frames) travel in ONE all_gather of a padded float64 tensor [runs_per_rank, 1 + 6
    + 2 T + 3] (run id first; pad rows = -1) -- a gather of its own: the others keep their shapes with the option off.  Rank 0
    forms the ratios with recon_metrics.summarise_raw (through tsdf.summarise_raw, which adds the counts and `options`) -> {run id:
    the record's "fusion" block}; the other ranks get {}."""
    from .utility import recon_metrics, tsdf
    rows = runs_per_rank(len(runs), world)
    width = 1 + recon_metrics.RAW_HEAD + 2 * len(thresholds) + len(tsdf.RAW_TAIL)
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        t[j, 0] = r["run_id"]
        t[j, 1:] = np.asarray(r["fusion_raw"], np.float64)
    collective = world > 1 or group_is_up()
    if collective:
        import torch.distributed as dist
        local = torch.from_numpy(t).to(collective_device(device))
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        t = torch.stack(buf).cpu().numpy().reshape(-1, width)
    if rank != 0:
        return {}
    return {int(row[0]): tsdf.summarise_raw(row[1:], thresholds, cap, options) for row in t if row[0] >= 0}


def gather_surface(results, runs, rank, world, device, spec):
    """The planning option `surface_metrics`: all ranks call this behind gather_results, and only when the option is on.  The raw
    float64 numbers of every run's cloud-to-mesh accuracy (results[i]["surface_raw"], utility/surface_metrics.py::pack_record: the
    raw cloud's sums, size and counts, the fused cloud's, has_fused and the mesh's three counts) travel in ONE all_gather of a padded
    float64 tensor [runs_per_rank, 1 + 2 (3 + T) + 4] (run id first; pad rows = -1) -- a gather of its own: the others keep their
    shapes with the option off.  spec: the normalised options (surface_metrics.option_spec).  Rank 0 forms the ratios with
    surface_metrics.summarise_record -> {run id: the record's "surface" block}; the other ranks get {}."""
    from .utility import surface_metrics
    rows = runs_per_rank(len(runs), world)
    width = 1 + 2 * (surface_metrics.RAW_HEAD + len(spec["thresholds"])) + len(surface_metrics.RECORD_TAIL)
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        t[j, 0] = r["run_id"]
        t[j, 1:] = np.asarray(r["surface_raw"], np.float64)
    collective = world > 1 or group_is_up()
    if collective:
        import torch.distributed as dist
        local = torch.from_numpy(t).to(collective_device(device))
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        t = torch.stack(buf).cpu().numpy().reshape(-1, width)
    if rank != 0:
        return {}
    return {int(row[0]): surface_metrics.summarise_record(row[1:], spec) for row in t if row[0] >= 0}


def gather_views(results, runs, rank, world, device, options):
    """The planning option `view_metrics`: all ranks call this behind gather_results, and only when the option is on.  The raw
    float64 counts and sums of every run's held-out views (results[i]["views_raw"]: up to options["views"] rows of
    utility/view_metrics.py::pack_raw's 9 numbers; a scene with fewer reachable poses has fewer) travel in ONE all_gather of a
    padded float64 tensor [runs_per_rank, 2 + 9 views] (run id, number of views, rows; pad rows = -1) -- a gather of its own: the
    others keep their shapes with the option off.  Rank 0 forms the ratios from them -> {run id: summarise_raw's dict with
    `options` (view_metrics.resolved_options: the same for every run)}; the other ranks get {}."""
    from .utility import view_metrics
    rows, per, n_max = runs_per_rank(len(runs), world), view_metrics.RAW_WIDTH, int(options["views"])
    width = 2 + n_max * per
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        raw = np.asarray(r["views_raw"], np.float64).reshape(-1, per)
        if raw.shape[0] > n_max:
            raise ValueError(f"gather_views: a run with {raw.shape[0]} views, above the option's {n_max}")
        t[j, 0], t[j, 1] = r["run_id"], raw.shape[0]
        t[j, 2:2 + raw.size] = raw.reshape(-1)
    collective = world > 1 or group_is_up()
    if collective:
        import torch.distributed as dist
        local = torch.from_numpy(t).to(collective_device(device))
        buf = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(buf, local)
        t = torch.stack(buf).cpu().numpy().reshape(-1, width)
    if rank != 0:
        return {}
    return {int(row[0]): view_metrics.summarise_raw(row[2:2 + int(row[1]) * per].reshape(int(row[1]), per), options)
            for row in t if row[0] >= 0}
