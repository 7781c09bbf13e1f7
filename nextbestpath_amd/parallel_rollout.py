"""Scene-parallel sharding of independent rollouts.

Each (scene, start pose) rollout is independent (next_best_path/testers/nbp_planning.py:414-467
runs them in nested loops on one GPU), so rank r takes runs r, r+W, r+2W, ... and the only
collectives are all_gathers of padded, fixed-width rows (run id first; pad rows = -1), a few KB over RCCL/xGMI, latency bound:
ONE of an fp32 tensor [runs_per_rank, n_poses + 3] holding (run id, final coverage, AUC, coverage curve) -- gather_results -- and
one of float64 sums and counts behind it for every record block that is on (testers/record_blocks.py; gather_reconstruction,
gather_reconstruction_curve, gather_views, gather_fusion, gather_surface, gather_fusion_mesh), from which rank 0 forms the ratios.  A block that is
off causes no collective, so every other gather keeps its shape.  One
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


def all_rows(local, world, device):
    """The half that every gather shares: this rank's padded rows (a numpy array [rows, width]) -> all ranks' rows [world rows, width]
    in rank order, through ONE all_gather on the collective's device where there is a process group (a 1-rank group still goes
    through the backend); without one, the rows themselves.  The dtype travels as it is."""
    if not (world > 1 or group_is_up()):
        return local
    import torch.distributed as dist
    mine = torch.from_numpy(local).to(collective_device(device))
    buf = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(buf, mine)
    return torch.stack(buf).cpu().numpy().reshape(-1, local.shape[1])


def gather_results(results, runs, rank, world, device, n_poses):
    """All ranks call this; every rank gets the list of {run_id, coverage, final, auc, scene, start}
    in run order (only the coverage metrics travel; pose histories stay in the per-rank results)."""
    allt = all_rows(pack_results(results, runs, n_poses, runs_per_rank(len(runs), world)), world, device)
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


def pack_raw_rows(results, rows, raw_key, width, per=None):
    """Local results -> padded float64 [rows, width]: the run id, then the run's raw numbers results[i][raw_key], which fill the row
    exactly; with `per`, the run id, the number of `per`-wide records the run has, and those records, as many as fit or fewer.
    Whatever is left, and every pad row, is -1.  Raw numbers that do not fit the width are a ValueError."""
    head = 1 if per is None else 2
    t = np.full((rows, width), -1.0, np.float64)
    for j, r in enumerate(results):
        raw = np.asarray(r[raw_key], np.float64).reshape(-1)
        if raw.size > width - head or (raw.size != width - head if per is None else raw.size % per):
            raise ValueError(f"{raw_key}: run {r['run_id']} has {raw.size} numbers, its row holds {width - head}"
                             + ("" if per is None else f" in records of {per}"))
        t[j, 0] = r["run_id"]
        if per is not None:
            t[j, 1] = raw.size // per
        t[j, head:head + raw.size] = raw
    return t


def gather_raw(results, runs, rank, world, device, raw_key, width, summarise, per=None):
    """The float64 gather of one record block: all ranks call it behind gather_results, and only when the block is on.  Every
    run's raw sums and counts (results[i][raw_key]) travel in ONE all_gather of pack_raw_rows' tensor [runs_per_rank, width] -- a
    gather of its own, so that the others keep their shapes with the block off.  Rank 0 forms the ratios from them -> {run id:
    summarise(raw)}, raw as the run's vector (with `per`: as its records [n, per]); the other ranks get {}."""
    t = all_rows(pack_raw_rows(results, runs_per_rank(len(runs), world), raw_key, width, per), world, device)
    if rank != 0:
        return {}
    if per is None:
        return {int(row[0]): summarise(row[1:]) for row in t if row[0] >= 0}
    return {int(row[0]): summarise(row[2:2 + int(row[1]) * per].reshape(int(row[1]), per)) for row in t if row[0] >= 0}


def gather_reconstruction(results, runs, rank, world, device, thresholds, cap):
    """The planning option `recon_metrics`: utility/recon_metrics.py::pack_raw's 6 + 2 T numbers per run -> {run id: summarise_raw's
    dict}."""
    from .utility import recon_metrics
    width = 1 + recon_metrics.RAW_HEAD + 2 * len(thresholds)
    return gather_raw(results, runs, rank, world, device, "reconstruction_raw", width,
                      lambda raw: recon_metrics.summarise_raw(raw, thresholds, cap))


def gather_reconstruction_curve(results, runs, rank, world, device, thresholds, cap, n_poses):
    """The planning option `recon_metrics` with `curve`: n_poses rows of pack_raw's 6 + 2 T numbers per run -> {run id:
    summarise_curve's dict}."""
    from .utility import recon_metrics
    per = recon_metrics.RAW_HEAD + 2 * len(thresholds)
    return gather_raw(results, runs, rank, world, device, "reconstruction_curve_raw", 1 + n_poses * per,
                      lambda raw: recon_metrics.summarise_curve(raw.reshape(n_poses, per), thresholds, cap))


def gather_fusion(results, runs, rank, world, device, thresholds, cap, options=None):
    """The planning option `fusion`: utility/tsdf.py::pack_raw's numbers per run (the reconstruction metrics' 6 + 2 T of the fused
    cloud, then observed_voxels, usable_voxels, frames) -> {run id: tsdf.summarise_raw's dict, with `options`}."""
    from .utility import recon_metrics, tsdf
    width = 1 + recon_metrics.RAW_HEAD + 2 * len(thresholds) + len(tsdf.RAW_TAIL)
    return gather_raw(results, runs, rank, world, device, "fusion_raw", width,
                      lambda raw: tsdf.summarise_raw(raw, thresholds, cap, options))


def gather_surface(results, runs, rank, world, device, spec):
    """The planning option `surface_metrics`: utility/surface_metrics.py::pack_record's 2 (3 + T) + 4 numbers per run (the raw
    cloud's, the fused cloud's, has_fused and the mesh's counts) -> {run id: summarise_record's dict}.  spec: the normalised options."""
    from .utility import surface_metrics
    width = 1 + 2 * (surface_metrics.RAW_HEAD + len(spec["thresholds"])) + len(surface_metrics.RECORD_TAIL)
    return gather_raw(results, runs, rank, world, device, "surface_raw", width,
                      lambda raw: surface_metrics.summarise_record(raw, spec))


def gather_fusion_mesh(results, runs, rank, world, device, spec, options=None):
    """The planning option `fusion` with `mesh`: utility/tsdf_mesh.py::pack_raw's 5 + 2 (3 + T) numbers per run (the mesh's counts and
    area, GT -> fused surface completeness, the vertices' accuracy against the GT mesh) -> {run id: tsdf_mesh.summarise_raw's dict,
    with `options`}.  spec: the thresholds, cap and cell (tsdf_mesh.metric_options); options: the volume's."""
    from .utility import tsdf_mesh
    return gather_raw(results, runs, rank, world, device, "fusion_mesh_raw", 1 + tsdf_mesh.raw_width(len(spec["thresholds"])),
                      lambda raw: tsdf_mesh.summarise_raw(raw, spec, options))


def gather_views(results, runs, rank, world, device, options):
    """The planning option `view_metrics`: up to options["views"] rows of utility/view_metrics.py::pack_raw's 9 numbers per run (a
    scene with fewer reachable poses has fewer: the row carries the count behind the run id) -> {run id: summarise_raw's dict with
    `options` (view_metrics.resolved_options: the same for every run)}.  More views than the option's are a ValueError."""
    from .utility import view_metrics
    per = view_metrics.RAW_WIDTH
    return gather_raw(results, runs, rank, world, device, "views_raw", 2 + int(options["views"]) * per,
                      lambda raw: view_metrics.summarise_raw(raw, options), per=per)
