"""The end-of-rollout blocks of a planning record, declared once: ALL_BLOCKS, in the record's order.  Each entry says which normalised
option turns the block on, its record key (the raw float64 numbers behind it sit beside it as key + "_raw" until they are gathered),
how to measure those numbers on a finished Rollout, the summariser's context -- from the options record, the parameters and
n_poses alone, so the same on every rank -- how to form the block from them, and which gather of parallel_rollout.py carries them.
nbp_planning.py::_result and collect_records are loops over this table ("Adding a record block")."""
from __future__ import annotations

from collections import namedtuple

from ..utility import recon_metrics, surface_metrics, tsdf, tsdf_mesh, view_metrics

# option, flag: on when the normalised spec `option` is not None (and its key `flag` set, where one is named).  measure(ro, n_poses,
# fused) -> the raw float64 array (fused: what ro.fused_cloud() gave, once per record; None without `fusion`).  context(opts,
# params, n_poses) -> ctx, a tuple; summarise(raw, *ctx) -> the block; parallel_rollout's function `gather`(results, runs, rank,
# world, device, *ctx) -> {run id: block} on rank 0; check(result, *ctx) raises where a run was not made with ctx
Block = namedtuple("Block", "option flag key measure context summarise gather check", defaults=(None,))


def _recon_context(opts, params, n_poses):
    spec = opts.recon_metrics or recon_metrics.option_spec(True)       # (`fusion` borrows recon_metrics' thresholds, or its defaults)
    return spec["thresholds"], spec["cap"]


def _check_views(result, options):
    if result["views"]["options"] != options:
        raise RuntimeError(f"view_metrics: run {result['run_id']} was evaluated with {result['views']['options']}, not {options}")


TAGS = "tags"                      # the place of a record's `policy`, `depth_noise`, `depth_filter`: behind the reconstruction entries
RECORD_ORDER = (
    Block("recon_metrics", None, "reconstruction",
          measure=lambda ro, n_poses, fused: ro.reconstruction_metrics(raw=True),
          context=_recon_context, summarise=recon_metrics.summarise_raw, gather="gather_reconstruction"),
    Block("recon_metrics", "curve", "reconstruction_curve",
          measure=lambda ro, n_poses, fused: ro.reconstruction_curve(n_poses, raw=True),
          context=lambda opts, params, n_poses: (*_recon_context(opts, params, n_poses), n_poses),
          summarise=lambda rows, thresholds, cap, n_poses: recon_metrics.summarise_curve(rows, thresholds, cap),
          gather="gather_reconstruction_curve"),
    TAGS,
    Block("view_metrics", None, "views",
          measure=lambda ro, n_poses, fused: ro.view_metrics(raw=True),
          context=lambda opts, params, n_poses: (view_metrics.resolved_options(opts.view_metrics, params.image_height,
                                                                               params.image_width, params.zfar),),
          summarise=view_metrics.summarise_raw, gather="gather_views", check=_check_views),
    Block("fusion", None, "fusion",
          measure=lambda ro, n_poses, fused: ro.fusion_metrics(raw=True, fused=fused),
          context=lambda opts, params, n_poses: (*_recon_context(opts, params, n_poses),
                                                 tsdf.resolved_options(opts.fusion, params.sensor_range)),
          summarise=tsdf.summarise_raw, gather="gather_fusion"),
    Block("surface_metrics", None, "surface",
          measure=lambda ro, n_poses, fused: ro.surface_metrics(raw=True, fused=fused),
          context=lambda opts, params, n_poses: (opts.surface_metrics,),
          summarise=surface_metrics.summarise_record, gather="gather_surface"),
    Block("fusion", "mesh", "fusion_mesh",
          measure=lambda ro, n_poses, fused: ro.fused_mesh_metrics(raw=True),
          context=lambda opts, params, n_poses: (tsdf_mesh.metric_options(opts.surface_metrics),
                                                 tsdf.resolved_options(opts.fusion, params.sensor_range)),
          summarise=tsdf_mesh.summarise_raw, gather="gather_fusion_mesh"),
)
ALL_BLOCKS = tuple(entry for entry in RECORD_ORDER if entry is not TAGS)
# the blocks that an observer option turns on by being on, with the curve beside its metric: what names the observer options
# (nbp_planning.OBSERVER_OPTIONS) and what tests/test_record_blocks_host.py pins.  `fusion_mesh` is an extra of `fusion`, behind them
BLOCKS = tuple(block for block in ALL_BLOCKS if block.key != "fusion_mesh")


def blocks_on(opts):
    """The blocks that the options record `opts` (its normalised specs by option name) turns on, in the record's order."""
    def on(block):
        spec = getattr(opts, block.option)
        return spec is not None and (block.flag is None or bool(spec.get(block.flag)))
    return tuple(block for block in ALL_BLOCKS if on(block))


def fill(record, blocks, entries, tags):
    """`record` gains entries(block) (a dict) for every block of `blocks`, and the dict `tags`, all in RECORD_ORDER."""
    for entry in RECORD_ORDER:
        if entry is TAGS:
            record.update(tags)
        elif entry in blocks:
            record.update(entries(entry))
    return record
