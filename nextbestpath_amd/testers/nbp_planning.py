"""Exploration rollout -- host-side mirror of next_best_path/testers/nbp_planning.py
(compute_nbp_trajectory :23-361, test_nbp_planning :364-516): same entry-point names, same
step order (S1-S14 of SURVEY.md section 3.1), same result-JSON schema; every tensor op of the
step is a kernel of libnbp_hip.so and nothing touches the disk inside the loop.

Per step: coverage (device counter, no sync) -> un-project the current frame -> fused 6-channel
map accumulation + trajectory channel -> replan test (mesh segment query) -> NBP forward ->
[replan: fusion, scoring, all-edges mask, host search] -> move (4 poses, ONE raster launch) ->
un-project the 4 supervision frames.  The cloud and its size live on the device.

Deliberate deviations (documented in DESIGN.md): the reference draws its 5 % sub-samples and
random headings from unseeded global generators (note R of the survey) -- here they are seeded;
obtain_depth's discarded outputs (long_term_utils.py:50-155) are not computed; the reference's
unbound-`next_idx` crash when no path exists (nbp_planning.py:255-258) becomes "turn in place".
"""
from __future__ import annotations

import json
import os
import random
import time
from types import SimpleNamespace

import numpy as np
import torch

from .. import _lib
from .. import parallel_rollout
from ..networks.nbp_model import NBP
from ..simulator import lockstep
from ..simulator import scene as sim_scene
from ..simulator.lockstep import N_POSES, RolloutState, _concurrent_streams, _settle_gc, setup_test_camera  # noqa: F401
from ..utility import augment, hipops
from ..utility import depth_filter as filter_options
from ..utility import depth_noise as noise_options
from ..utility import recon_metrics as recon_options
from ..utility import surface_metrics as surface_options
from ..utility import tsdf as fusion_options
from ..utility import utils as hu
from ..utility import view_metrics as view_options
from ..utility.long_term_utils import LatticePlanner, compute_auc
from . import record_blocks

# Rollout.step: the step's forward on a stream of its own, behind the map stage by an event.  The reference runs the network at
# every step and reads its output only when it replans (nbp_planning.py:166 / :252): a step that does not replan goes on to the move
# and the next observation while its forward (every kernel of it, on the same input) is still running.  0 = everything in stream order.
_STEP_OVERLAP = _lib.tune("NBP_STEP_OVERLAP", "1") == "1"


_UNSET = object()


def _set_symmetry_ensemble(nbp, params, spec=_UNSET):
    """The planning option `symmetry_ensemble` (None, a name of utility/augment.py::ENSEMBLES or a list of op codes) goes onto the
    network the rollouts evaluate: the keyword where given, else the params' key where present, else the network keeps its own."""
    if spec is _UNSET:
        spec = getattr(params, "symmetry_ensemble", _UNSET)
    if spec is not _UNSET:
        nbp.symmetry_ensemble = spec        # (a policy refuses anything but None: ValueError)


def _wants_maps(nbp):
    """Is `nbp` a policy that reads the six-channel map stack (testers/frontier_policy.py) and not the network input?"""
    return getattr(nbp, "wants_maps6", False)


def _policy_forward(policy, maps6):
    """The policy branch of a step's forward: the planner's two inputs from the map stack [B,6,S,S].  Never entered with a network."""
    return policy.forward_maps(maps6)


class Rollout(lockstep.LockstepRollout):
    """One exploration rollout, steppable (bench.py times K consecutive ``step()`` calls)."""

    def __init__(self, params, nbp, camera, gt_scene_pc, mesh, mesh_for_check, y_bins, device, state=None, seed=0,
                 grid=256, symmetry_ensemble=_UNSET, recon_metrics=None, view_metrics=None, fusion=None, surface_metrics=None):
        self.params, self.nbp, self.camera, self.mesh, self.mesh_for_check = params, nbp, camera, mesh, mesh_for_check
        _set_symmetry_ensemble(nbp, params, symmetry_ensemble)
        self.y_bins, self.device = y_bins, device
        # the reference hard-codes 256 / 64 / +-40 (nbp_planning.py:43-45); other grids keep 0.3125 units per pixel
        self.S, self.V, self.grid_range = grid, grid // 4, (-40 * grid // 256, 40 * grid // 256)
        self.st = state or RolloutState(device, grid=grid)
        # a state taken over from an earlier rollout may still have that rollout's side-stream forwards in flight on its input
        # buffers: this stream waits for them before the state is overwritten
        self._wait_forwards()
        self.st.cloud_count.zero_()
        self.st.coverage_counts.zero_()
        self.st.frames_appended = 0
        self.st.frames_filed = 0
        # the step's maps come from the tile-binned shadow copy of the cloud (utils.CloudBins; bit-identical maps)
        vh = np.asarray(mesh.verts_host, np.float32)
        lo, hi = (float(vh[:, 0].min()), float(vh[:, 2].min())), (float(vh[:, 0].max()), float(vh[:, 2].max()))
        b = self.st.bins
        if b is None or (tuple(b.lo), tuple(b.hi), b.capacity) != (lo, hi, self.st.cloud.shape[0]):
            self.st.bins = hu.CloudBins(lo, hi, self.st.cloud.shape[0], device)
        else:
            b.reset()                     # the cloud starts from zero points again
        self.rng = random.Random(seed)
        self.planner = LatticePlanner(camera, mesh_for_check, device, self.V, self.S, self.grid_range, rng=self.rng)
        self.gt = gt_scene_pc.contiguous()
        self.bbox = (self.gt.min(0).values.tolist(), self.gt.max(0).values.tolist())
        self.cov_plan = hipops.CoveragePlan(self.gt, 1.0, 2, self.bbox)          # GT sorted once per rollout
        # the planning option `recon_metrics` (None = off: nothing is built or launched; True; a dict thresholds / cap / cell / curve)
        self.recon_spec = recon_options.option_spec(recon_metrics)
        self.recon, self.recon_curve, self._curve_frames = None, None, 0
        if self.recon_spec is not None:
            kw = recon_options.metrics_kwargs(self.recon_spec)
            self.recon = hipops.ReconMetrics(self.gt, self.bbox, **kw)
            if self.recon_spec.get("curve"):    # ... with `curve`: the same metrics after every step, updated incrementally (pre)
                self.recon_curve = hipops.ReconCurve(self.gt, self.bbox, **kw, plan=self.recon.plan)
        self._defaults = {}                 # metrics objects built for a direct call on a rollout without the option (_metrics)
        # the planning option `view_metrics` (None = off: nothing is built or launched; True; a dict of utility/view_metrics.py): the
        # coloured cloud rendered from held-out lattice poses against the mesh, once, at the rollout's end
        self.view_spec = view_options.option_spec(view_metrics)
        # where the rollout starts: the root of the held-out poses
        self._start_ijk = None if camera.cam_idx is None else tuple(int(v) for v in camera.cam_idx[:3])
        self.views = self._build_views(self.view_spec) if self.view_spec is not None else None
        # the planning option `fusion` (None = off: nothing is allocated, launched, gathered or written; True; a dict of
        # utility/tsdf.py): every frame the rollout un-projects also goes into a TSDF volume over the GT bounds, an observer like
        # recon_metrics -- nothing of the step reads it -- whose fused surface cloud is judged once, at the rollout's end
        self.fusion_spec = fusion_options.option_spec(fusion)
        self.fusion = None
        if self.fusion_spec is not None:
            self.fusion = hipops.TSDFVolume(self.bbox, fusion_options.resolved_options(self.fusion_spec, params.sensor_range), device)
        # the planning option `surface_metrics` (None = off: nothing is built, launched, gathered or written; True; a dict of
        # utility/surface_metrics.py): the cloud's accuracy against the GT MESH, not the GT sample, once, at the rollout's end; the
        # mesh's triangle grid is built here (one read-back of its size)
        self.surface_spec = surface_options.option_spec(surface_metrics)
        self.surface = None if self.surface_spec is None else hipops.SurfaceMetrics(mesh, **self.surface_spec)
        self.path, self.path_record = [], 0
        self.collision_list, self.passable_list, self.idx_history = [], [], []
        self.step_seed = seed * 1_000_003
        self.pose_i = 0
        self.n_replans = 0
        _settle_gc()

    # The step is split in enqueue-only halves so that MultiRollout can batch the NBP forward of several
    # rollouts and share one stream synchronisation per step; step() is the single-rollout composition.
    def pre(self, net_in=None):
        """S2-S8: coverage, un-projection of the current frame, maps, replan decision.  No host sync."""
        st = self.st
        net_in = st.net_in if net_in is None else net_in
        # the bins are in step with the cloud (every frame so far was filed): this step's un-projection files its points too and
        # clears the maps, and the build below is the page launch alone (nbp_step_maps_prefiled_f32; bit-identical maps)
        prefiled = st.frames_filed == st.frames_appended
        self.count_coverage()
        self.update_recon_curve()          # (option `recon_metrics` with `curve`: row pose_i = the cloud the coverage just saw)
        self.unproject(lockstep.CURRENT, True, clear=(st.maps6, net_in[0, 4]) if prefiled else None)
        prefiled = prefiled and st.frames_filed == st.frames_appended
        # S5-S7 in one call: six maps, trajectory channel, network input
        full_pc, n_upper, n_dev, pose, y_bins, traj_dev, n_old, fresh, bins = self.maps_item()
        hu.step_maps(full_pc, pose, y_bins, self.S, self.grid_range, traj_dev, n_old, fresh, st.maps6, net_in[0], n_dev=n_dev,
                     bins=bins, n_upper=n_upper, prefiled=prefiled)
        st.frames_filed = st.frames_appended       # (a two-launch build files whatever the store had not seen)
        self.traj_img = net_in[0, 4]               # stays valid until this rollout's next pre()
        self.pre_decide()

    def pre_decide(self):
        """S8: does this step replan?  Host only."""
        camera, pose_i = self.camera, self.pose_i
        path = self.path
        if pose_i == 0 or not path or self.path_record + 1 > len(path):
            self.need_replan = True
        else:
            nxt = path[self.path_record]
            self.need_replan = self.planner.edge_hits_mesh(camera.cam_idx[:3], nxt[:3])
            if self.need_replan:
                cur3, nxt3 = list(camera.cam_idx[:3]), list(nxt[:3])
                self.collision_list += [[cur3, nxt3], [nxt3, cur3], list(path[-1][:3])]
        if len(self.idx_history) >= 2:
            p1, p2 = list(self.idx_history[-1][:3]), list(self.idx_history[-2][:3])
            self.passable_list += [[p1, p2], [p2, p1]]

    def plan_enqueue(self, out1, out2):
        if self.need_replan:
            self.n_replans += 1
            self.path_record = 0
            self.planner.replan_enqueue(self.pose, out1, out2, self.st.maps6, self.traj_img, self.collision_list)

    def plan_finish(self):
        if self.need_replan:
            self.path = self.planner.replan_finish(self.collision_list, self.passable_list)

    def post(self):
        """S10-S14: next pose, move (4 poses, one raster launch), un-project the supervision frames."""
        self.camera.move_and_capture(self.mesh, self.post_choose())
        self.unproject(lockstep.SUPERVISION, True)
        self.post_finish()

    def post_choose(self):
        """S10: the next lattice pose (host only)."""
        camera, path = self.camera, self.path
        if not path or self.path_record >= len(path):
            next_idx = list(camera.cam_idx)
            next_idx[4] = self.rng.randrange(8)
            path = []
        else:
            next_idx = list(path[self.path_record])
            if tuple(next_idx) in {tuple(h) for h in self.idx_history}:
                next_idx[4] = self.rng.randrange(8)
        self.path = path
        self.idx_history.append(tuple(camera.cam_idx))
        return next_idx

    def post_finish(self):
        self.path_record += 1
        self.pose_i += 1

    def step(self):
        policy = _wants_maps(self.nbp)
        static = None if policy else getattr(self.nbp, "forward_static", None)
        if static is not None and _STEP_OVERLAP and not self.nbp.training:
            return self._step_forward_on_its_own_stream(static)
        self.pre()
        with torch.no_grad():          # S9: one NBP forward per step (the reference also runs it without replanning, :252)
            if policy:                 # (in stream order: the map stack is one buffer, the next step's map stage clears it)
                out1, out2 = _policy_forward(self.nbp, self.st.maps6[None])
            else:
                # net_in is a persistent tensor: the ~60 launches of a B = 1 forward replay as one hipGraph (bit-identical outputs)
                out1, out2 = static(self.st.net_in) if static is not None else self.nbp(self.st.net_in)
        self.plan_enqueue(out1, out2)
        if self.need_replan:
            torch.cuda.current_stream().synchronize()
        self.plan_finish()
        self.post()

    def _step_forward_on_its_own_stream(self, static):
        """step() with the forward (the replayed hipGraph of this input buffer) on a side stream: same kernels, same inputs, same
        results; only a replanning step waits for it.  Networks only: a policy reads the map stack, which is not double-buffered,
        so step() keeps it in stream order."""
        if _wants_maps(self.nbp):
            raise RuntimeError("a policy's forward stays in stream order (Rollout.step)")
        st = self.st
        ov = st.forward_overlap()
        slot = self.pose_i & 1
        main = torch.cuda.current_stream(self.device)
        net_in, fwd = ov["net_in"][slot], ov["streams"][slot]
        if ov["used"][slot]:
            main.wait_event(ov["done"][slot])          # the forward of two steps ago has read this buffer
        st.net_in = net_in                             # (the input of the latest step, whichever buffer it is)
        self.pre(net_in)
        ov["maps"][slot].record(main)
        with torch.cuda.stream(fwd), torch.no_grad():
            fwd.wait_event(ov["maps"][slot])
            out1, out2 = static(net_in)
            ov["done"][slot].record(fwd)
        ov["used"][slot] = True
        if self.need_replan:
            main.wait_event(ov["done"][slot])
            self.plan_enqueue(out1, out2)
            main.synchronize()
            self.plan_finish()
        self.post()

    def _wait_forwards(self):
        ov = getattr(self.st, "_overlap", None)
        if ov is not None:
            main = torch.cuda.current_stream(self.device)
            for k, (used, ev) in enumerate(zip(ov["used"], ov["done"])):
                if used:
                    main.wait_event(ev)
                    ov["used"][k] = False          # (a later step on this slot records the event again before anyone waits on it)

    def finish(self):
        """The caller's stream waits for the forwards still in flight (before the network's weights or the state are reused).
        Idempotent; coverage_evolution() -- what every driver ends a rollout with -- calls it, and a Rollout that takes over a used
        state waits in its constructor, so a loop over step() that never calls finish() is safe as well."""
        self._wait_forwards()

    def _metrics(self, name):
        """The rollout's own metrics object `name` ("recon", "views", "surface"), or, where it was built with that option off, one
        with the option's defaults: made at the first call and kept apart from self.<name>, so that the rollout keeps reporting the
        option as off."""
        build = {"recon": lambda: hipops.ReconMetrics(self.gt, self.bbox, **recon_options.option_spec(True)),
                 "views": lambda: self._build_views(view_options.option_spec(True)),
                 "surface": lambda: hipops.SurfaceMetrics(self.mesh, **surface_options.option_spec(True))}
        if getattr(self, name) is None and name not in self._defaults:
            self._defaults[name] = build[name]()
        return getattr(self, name) or self._defaults[name]

    def _counted(self, fused):
        """(points, n) of fused_cloud() -> (points, n as a device count) for the metrics' kernels, which take a buffer of at least
        one row: an empty cloud goes as one dummy row, and the count says that none is valid."""
        points, n = fused
        if n == 0:
            points = torch.zeros(1, 3, dtype=torch.float32, device=self.device)
        return points, torch.full((1,), n, dtype=torch.int64, device=self.device)

    def reconstruction_metrics(self, raw=False):
        """Reconstruction quality of the WHOLE cloud so far (no sub-sampling) against the GT surface: the dict of
        utility/recon_metrics.py::summarise (accuracy, completeness, Chamfer distance, precision / recall / F-score per threshold),
        or with raw=True its raw float64 sums and counts (recon_metrics.pack_raw: what travels between ranks).  Evaluated on the
        device (hipops.ReconMetrics: both nearest-neighbour directions and their summaries, no host synchronisation), read back
        with one copy.  With the rollout's own `recon_metrics` option, or the defaults where it was built without one."""
        self.finish()
        rec = self._metrics("recon")
        rec.evaluate(self.st.cloud, self.st.cloud_count)
        return rec.raw() if raw else rec.summary()

    def _build_views(self, spec):
        """hipops.ViewMetrics of the held-out poses of `spec` (view_metrics.choose_views over the planner's lattice from the
        rollout's start position), with the options it is made with as `.options`."""
        cam, pl = self.camera, self.planner
        opts = view_options.resolved_options(spec, cam.image_height, cam.image_width, self.params.zfar)
        picks = view_options.choose_views(pl.nbrs, pl.mesh_hit, pl.node_index[self._start_ijk], opts["views"], opts["seed"])
        cams = np.stack([cam.cam12_of_pose(cam.pose_from_idx((*pl.idx3_list[node], 2, heading))) for node, heading in picks])
        vm = hipops.ViewMetrics(self.mesh, cams, opts["height"], opts["width"], radius=opts["radius"],
                                depth_tolerance=opts["depth_tolerance"], z_far=opts["z_far"], ambient=cam.ambient,
                                contrast=cam.contrast_factor, colours=cam.renders_colours)
        vm.options = opts
        return vm

    def view_metrics(self, raw=False):
        """Held-out view metrics of the WHOLE coloured cloud so far: the dict of utility/view_metrics.py::summarise_raw (the share of
        the visible surface that is filled at the right depth, holes, leaks, floaters, depth error and PSNR, with the options used),
        or with raw=True the float64 rows [views, 9] behind it (what travels between ranks).  Evaluated on the device
        (hipops.ViewMetrics: splat and statistics, no host synchronisation), read back with one copy.  With the rollout's own
        `view_metrics` option, or the defaults where it was built without one."""
        self.finish()
        vm = self._metrics("views")
        rgb = self.st.cloud_rgb if self.camera.renders_colours else None
        vm.evaluate(self.st.cloud, rgb, self.st.cloud_count)
        return vm.raw() if raw else vm.summary(vm.options)

    def fused_cloud(self):
        """(points fp32 [n,3] on the device, n): the surface cloud of the rollout's TSDF volume (the option `fusion`), in
        utility/tsdf.py::extract's order.  Reads the point count back: for the rollout's end, not for the step."""
        if self.fusion is None:
            raise RuntimeError("fused_cloud: the rollout was built without the option `fusion`")
        self.finish()
        return self.fusion.extract()

    def fusion_metrics(self, raw=False, fused=None):
        """Reconstruction quality of the FUSED cloud against the GT surface, by the metrics that judge the raw cloud
        (hipops.ReconMetrics with the rollout's `recon_metrics` option, or that option's defaults): utility/tsdf.py::summarise_raw's
        dict -- recon_metrics.summarise's entries (n_points = the fused points) with observed_voxels, usable_voxels, frames and the
        volume's options -- or with raw=True the float64 vector behind it (tsdf.pack_raw: what travels between ranks).  `fused`:
        what fused_cloud() returned, where the caller has extracted it already."""
        fused = self.fused_cloud() if fused is None else fused
        rec = self._metrics("recon")
        rec.evaluate(*self._counted(fused))
        st = self.fusion.stats()
        row = fusion_options.pack_raw(rec.raw(), st["observed_voxels"], st["usable_voxels"], self.fusion.frames)
        return row if raw else fusion_options.summarise_raw(row, rec.thresholds, rec.cap, self.fusion.options)

    def fused_mesh(self):
        """(verts fp32 [V,3], faces int32 [F,3] on the device): the triangle mesh of the rollout's TSDF volume (the option `fusion`),
        utility/tsdf_mesh.py::mesh's.  Reads the two counts back: for the rollout's end, not for the step."""
        if self.fusion is None:
            raise RuntimeError("fused_mesh: the rollout was built without the option `fusion`")
        self.finish()
        return self.fusion.mesh()

    def fused_mesh_metrics(self, raw=False):
        """The fused MESH against the GT (the option `fusion` with `mesh`; hipops.FusedMeshMetrics): its counts and area, GT sample ->
        fused surface completeness and the accuracy of its vertices against the GT mesh, with the thresholds, cap and cell of the
        rollout's `surface_metrics` option, or that option's defaults: utility/tsdf_mesh.py::summarise_raw's dict, or with raw=True the
        float64 vector behind it (tsdf_mesh.pack_raw: what travels between ranks)."""
        if self.fusion is None:
            raise RuntimeError("fused_mesh_metrics: the rollout was built without the option `fusion`")
        self.finish()
        sm = self._metrics("surface")
        fm = hipops.FusedMeshMetrics(self.gt, sm, sm.thresholds, sm.cap, sm.cell)      # (holds no device state of its own)
        row = fm.evaluate(self.fusion)
        return row if raw else fm.summary(self.fusion.options)

    def surface_metrics(self, raw=False, fused=None):
        """Accuracy of the WHOLE cloud so far against the surface of the GT mesh (exact point-to-triangle distances, no GT sample
        in between), and with the option `fusion` of the fused cloud too: utility/surface_metrics.py::summarise_record's dict
        {"cloud": n_points, cap, accuracy_mean, accuracy_rmse, thresholds = [{threshold, precision}]; "fused": the same (only with
        fusion); "mesh": {faces, faces_used, entries}; "options"}, or with raw=True the float64 vector behind it (pack_record: what
        travels between ranks).  Evaluated on the device (hipops.SurfaceMetrics), read back with one copy per cloud.  `fused`: what
        fused_cloud() returned, where the caller has extracted it already.  With the rollout's own `surface_metrics` option, or the
        defaults where it was built without one."""
        self.finish()
        sm = self._metrics("surface")
        sm.evaluate(self.st.cloud, self.st.cloud_count)
        cloud_raw, fused_raw = sm.raw(), None
        if self.fusion is not None:
            sm.evaluate(*self._counted(self.fused_cloud() if fused is None else fused))
            fused_raw = sm.raw()
        row = surface_options.pack_record(cloud_raw, fused_raw, sm.mesh_block())
        return row if raw else surface_options.summarise_record(row, {"thresholds": sm.thresholds, "cap": sm.cap, "cell": sm.cell})

    def reconstruction_curve(self, n, raw=False):
        """The per-step reconstruction curve (the option `recon_metrics` with `curve`): entry s is the metric of the WHOLE cloud as
        step s found it -- the cloud that coverage[s] was counted on -- from the incremental device state (hipops.ReconCurve), read
        back with one copy: the dict of lists of utility/recon_metrics.py::summarise_curve, or with raw=True the float64 rows
        [n, 6 + 2 T] behind it (what travels between ranks)."""
        if self.recon_curve is None:
            raise RuntimeError("reconstruction_curve: the rollout was built without recon_metrics = {..., 'curve': True}")
        self.finish()
        return self.recon_curve.raw(n) if raw else self.recon_curve.curve(n)

    def coverage_evolution(self, n):
        self.finish()
        counts = self.st.coverage_counts[:n].cpu().numpy()
        G = np.float32(len(self.gt))
        return [float(np.float32(c) / G) for c in counts[:, 0]]


class MultiRollout:
    """R independent rollouts (different scenes / start poses) on one GPU ("B_rollout
    concurrent rollouts per rank").  They are split in two groups that are software-pipelined: while the GPU
    runs one group's batched NBP forward (B = R/2 in the GEMM M dimension) the host finishes the other
    group's replanning (event wait + search) and enqueues its move / raster / un-projection, so neither
    side idles.  Each group has its own HIP stream: the small latency-bound kernels of one group's step (coverage,
    un-projection, map accumulation, raster, planner) run underneath the other group's convolutions instead of
    in front of them.  Each rollout's results are identical to running it alone (tests/test_gpu_rollout.py)."""

    def __init__(self, rollouts, nbp, device, grid=None, streams=True, n_groups=None, elide_dead_forward=False,
                 symmetry_ensemble=_UNSET):
        self.rollouts, self.nbp = list(rollouts), nbp
        _set_symmetry_ensemble(nbp, getattr(self.rollouts[0], "params", None), symmetry_ensemble)
        # The reference runs the network at every step and uses its output only when it replans (nbp_planning.py:166 / :252).
        # Default (False): every rollout's map goes through the forward at every step, as there.  True (reported beside the
        # headline, never as it): only the replanning rollouts' maps are forwarded -- same trajectories, same coverage
        # (tests/test_gpu_rollout.py::test_dead_forward_elision_changes_nothing).
        self.elide_dead_forward = bool(elide_dead_forward)
        self._sub = {}
        self.device, self._packed = device, None
        grid = grid or self.rollouts[0].S
        R = len(self.rollouts)
        # two pipeline groups, and more once a group would exceed 24 rollouts (measured: 48 = 2 x 24 is the best split of one
        # GPU; groups of 30+ lose 15 % in bench.py's configuration, 3 x 24 is level with 2 x 24)
        n_groups = n_groups or int(_lib.tune("NBP_ROLLOUT_GROUPS", "0")) or max(2, (R + 23) // 24)
        n_groups = max(1, min(n_groups, R))
        per = (R + n_groups - 1) // n_groups
        self.groups = [self.rollouts[i:i + per] for i in range(0, R, per)]
        self.net_in = [torch.zeros(len(g), 5, grid, grid, dtype=torch.float32, device=device) for g in self.groups]
        # the rollouts' map stacks as slices of one tensor per group: each latency-bound stage of the group's step is ONE batched
        # launch.  False: the per-rollout composition (Rollout.pre / plan_enqueue / post, one event per rollout), the reference of
        # tests/test_gpu_rollout.py::test_group_larger_than_the_batched_kernels_hold
        self.batched = True
        self.maps6 = [torch.zeros(len(g), 6, grid, grid, dtype=torch.float32, device=device) for g in self.groups]
        self._out1_pin = [torch.empty(len(g), 8, grid // 4, grid // 4, dtype=torch.float32).pin_memory() for g in self.groups]
        self._plan_event = [None] * len(self.groups)
        for g, m6 in zip(self.groups, self.maps6):
            for i, r in enumerate(g):
                r.st.maps6 = m6[i]
        # the replanning results of a group's rollouts as rows of ONE buffer pair per group (one device -> host copy per group and
        # step); rollouts whose lattices differ in size keep their own buffers
        self._res = []
        for g in self.groups:
            nb = {r.planner.result_bytes() for r in g}
            if len(nb) == 1:
                n = nb.pop()
                devb = torch.empty(len(g), n, dtype=torch.uint8, device=device)
                pinb = torch.empty(len(g), n, dtype=torch.uint8).pin_memory()
                for i, r in enumerate(g):
                    r.planner.share_result_buffers(devb[i], pinb[i])
                self._res.append((devb, pinb))
            else:
                self._res.append(None)
        self.inflight = [False] * len(self.groups)
        # Streams.  One HIP stream per group carries the group's small kernels and its batched forward.  (Side streams for the
        # rollouts' small kernels were measured and rejected, HISTORY.md: every cross-stream event dependency costs more than the
        # overlap returns, and the convolutions hold every CU's registers and LDS anyway.)
        main = torch.cuda.current_stream(device)
        self.stream_check = None
        if streams and len(self.groups) >= 2:
            self.streams, self.stream_check = _concurrent_streams(device, len(self.groups))
            for st in self.streams:
                st.wait_stream(main)          # the rollouts were built on the caller's stream
        else:
            self.streams = [main for _ in self.groups]
        self.ev_plan = [[torch.cuda.Event() for _ in g] for g in self.groups]

    def _launch(self, gi):
        grp, net_in = self.groups[gi], self.net_in[gi]
        # a single stream guard around the whole group (a guard per rollout is ~10 us of host time)
        with torch.cuda.stream(self.streams[gi]):
            if self.batched:
                self._pre_group(gi)
            else:
                for i, r in enumerate(grp):
                    r.pre(net_in[i:i + 1])
            rows = None
            if self.elide_dead_forward and self.batched and self._packed is not None:
                out1, out2, rows = self._forward_replanning_only(gi)
            else:
                with torch.no_grad():
                    if _wants_maps(self.nbp):          # a policy gets the group's map stacks, not the network input
                        out1, out2 = _policy_forward(self.nbp, self.maps6[gi])
                    else:
                        out1, out2 = self._forward(net_in)
            if self.batched:
                self._plan_group(gi, out1, out2, rows)
            else:
                for i, r in enumerate(grp):
                    r.plan_enqueue(out1[i], out2[i])
                    self.ev_plan[gi][i].record()
        self.inflight[gi] = True

    def _pre_group(self, gi):
        """Rollout.pre for every rollout of the group, each latency-bound stage as ONE batched launch (identical results)."""
        grp, net_in = self.groups[gi], self.net_in[gi]
        hipops.coverage_count_batch([r.coverage_item() for r in grp])
        curves = [it for it in (r.recon_curve_item() for r in grp) if it is not None]
        if curves:                         # the option `recon_metrics` with `curve`: ONE call for the group
            hipops.recon_curve_update_batch(curves)
        lockstep.unproject_group(grp, lockstep.CURRENT, True)
        hu.step_maps_batch([r.maps_item() for r in grp], grp[0].S, grp[0].grid_range, self.maps6[gi], net_in)
        for i, r in enumerate(grp):
            r.traj_img = net_in[i, 4]
            r.pre_decide()

    def _forward_replanning_only(self, gi):
        """elide_dead_forward: the forward over the maps of the rollouts that replan this step only -> (out1, out2, {rollout
        index in the group: row}); (None, None, {}) when none does.  The rows are gathered on the device (index list through a
        pinned buffer: no pageable copy in the loop); the workspace is the full group's."""
        from ..networks import packing
        grp, net_in = self.groups[gi], self.net_in[gi]
        need = [i for i, r in enumerate(grp) if r.need_replan]
        if not need:
            return None, None, {}
        if len(need) == len(grp):
            with torch.no_grad():
                out1, out2 = self._forward(net_in)
            return out1, out2, None
        st = self._sub.get(gi)
        if st is not None and st["packed"] is not self._packed:     # a new pack (weights, precision, ensemble): other sizes
            st = None
        if st is None:
            n, S = net_in.shape[0], net_in.shape[-1]
            nbytes = max(packing.forward_workspace_bytes(self._packed, b, S) for b in range(1, n + 1))
            st = self._sub[gi] = {"packed": self._packed,"pin": [torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(4)], "k": 0,
                                  "idx": torch.zeros(n, dtype=torch.int64, device=self.device), "x": torch.empty_like(net_in),
                                  "ws": torch.empty(nbytes, dtype=torch.uint8, device=self.device)}
        k = len(need)
        pin = st["pin"][st["k"] % 4]
        st["k"] += 1
        pin[:k] = torch.tensor(need, dtype=torch.int64)
        st["idx"][:k].copy_(pin[:k], non_blocking=True)
        x = st["x"][:k]
        torch.index_select(net_in, 0, st["idx"][:k], out=x)
        with torch.no_grad():
            out1, out2 = packing.forward_packed(self._packed, x, ws=st["ws"])
        return out1, out2, {i: row for row, i in enumerate(need)}

    def _plan_group(self, gi, out1, out2, rows=None):
        """Rollout.plan_enqueue for the group: the replanning rollouts' GPU half in two launches, their results in one copy each
        plus ONE copy of the group's value maps; one event for all of them.  rows: rollout index -> row of out1 / out2 (None:
        the identity)."""
        grp = self.groups[gi]
        need = [(i, r) for i, r in enumerate(grp) if r.need_replan]
        if need:
            r0 = grp[0]
            pin = self._out1_pin[gi]
            items = []
            row = (lambda i: i) if rows is None else rows.__getitem__
            for i, r in need:
                r.n_replans += 1
                r.path_record = 0
                items.append(r.planner.replan_item(r.pose, out1[row(i)].reshape(8, r.V, r.V), out2[row(i)].reshape(r.S, r.S), r.st.maps6,
                                                   r.traj_img.reshape(r.S, r.S), r.collision_list))
            hipops.replan_batch(items, r0.S, r0.V, r0.grid_range)
            pin[:out1.shape[0]].copy_(out1, non_blocking=True)
            if self._res[gi] is not None:
                self._res[gi][1].copy_(self._res[gi][0], non_blocking=True)        # every rollout's (scores, valid, blocked) rows at once
            for i, r in need:
                r.planner.replan_copy_back(r.pose, pin[row(i)].reshape(8, r.V, r.V))
        ev = self.ev_plan[gi][0]
        ev.record()
        self._plan_event[gi] = ev

    def _post_group(self, grp):
        """Rollout.post for the rollouts of a group: their moves are rendered in ONE batched rasteriser call and their
        supervision frames un-projected in one (identical results)."""
        lockstep.render_moves(grp, [r.post_choose() for r in grp])
        lockstep.unproject_group(grp, lockstep.SUPERVISION, True)
        for r in grp:
            r.post_finish()

    def _forward(self, net_in):
        """The rollouts evaluate a frozen network: its packed weights are looked up (and their staleness checked: 327 tensor
        versions) once per lock-step, not once per forward."""
        if self._packed is None:
            return self.nbp(net_in)
        from ..networks import packing
        return packing.forward_packed(self._packed, net_in)

    def _complete(self, gi):
        grp = self.groups[gi]
        if self._plan_event[gi] is not None:
            if any(r.need_replan for r in grp):
                self._plan_event[gi].synchronize()     # one event for the group's batched replan results
            self._plan_event[gi] = None
        else:
            for i, r in enumerate(grp):
                if r.need_replan:
                    self.ev_plan[gi][i].synchronize()      # the GPU keeps running whatever was queued after the event
        with torch.cuda.stream(self.streams[gi]):
            for r in grp:
                r.plan_finish()
            if self.batched:
                self._post_group(grp)
            else:
                for r in grp:
                    r.post()
        self.inflight[gi] = False

    def step(self):
        """One exploration step of every rollout (completions are deferred: a group is finished right after the
        next group has been launched, so the GPU always has another group's forward queued)."""
        G = len(self.groups)
        ensure = getattr(self.nbp, "_ensure_packed", None)
        self._packed = ensure(self.device) if ensure is not None and not self.nbp.training else None
        for gi in range(G):
            if self.inflight[gi]:
                self._complete(gi)
            self._launch(gi)
            prev = (gi - 1) % G
            if G >= 2 and self.inflight[prev] and prev != gi:
                self._complete(prev)
        if G == 1:
            self._complete(0)

    def flush(self):
        for gi in range(len(self.groups)):
            if self.inflight[gi]:
                self._complete(gi)
        main = torch.cuda.current_stream()
        for st in set(self.streams):
            if st is not main:
                main.wait_stream(st)           # later work on the caller's stream sees every rollout's results


def compute_nbp_trajectory(params, nbp, camera, gt_scene_pc, mesh, mesh_for_check, n_pieces, y_bins, device,
                           test_resolution=0.05, use_perfect_depth_map=True, n_poses=N_POSES, state=None, seed=0):
    """Same name / leading arguments / return tuple as the reference (nbp_planning.py:23-361)."""
    t1 = time.time()
    nbp.eval()
    ro = Rollout(params, nbp, camera, gt_scene_pc, mesh, mesh_for_check, y_bins, device, state, seed)
    for _ in range(n_poses):
        ro.step()
    ro.finish()
    coverage_evolution = ro.coverage_evolution(n_poses)
    n_cloud = int(ro.st.cloud_count.item())
    print("Time: ", time.time() - t1)
    colors = ro.st.cloud_rgb[:n_cloud] if camera.renders_colours else None
    return coverage_evolution, camera.X_cam_history, camera.V_cam_history, ro.st.cloud[:n_cloud], colors


# the option keys of the configs/test/ file load_params read last (a file with the NBP options: `nbp_weights`), each _UNSET where the
# file has none; the entry script passes test_nbp_planning the options it knows by keyword, and these reach it here.  In the order
# in which resolve_options checks them
_test_config = dict.fromkeys(("policy", "symmetry_ensemble", "recon_metrics", "depth_noise", "depth_filter", "view_metrics", "fusion",
                             "surface_metrics"), _UNSET)


def load_params(path):
    """macarons/utility/utils.py:44-83: JSON -> attribute object, `_section` keys flattened away."""
    with open(path) as fh:
        raw = json.load(fh)

    def flat(d, out):
        for k, v in d.items():
            if isinstance(v, dict) and k.startswith("_"):
                flat(v, out)
            else:
                out[k] = v
        return out

    class Params:
        pass

    p = Params()
    for k, v in flat(raw, {}).items():
        setattr(p, k, v)
    if hasattr(p, "nbp_weights"):
        for key in _test_config:
            _test_config[key] = getattr(p, key, _UNSET)
    return p


def list_runs(dataset, params):
    """Flattened (scene x start pose) list: the unit of scene-parallel sharding."""
    runs = []
    for si in range(len(dataset)):
        sd = dataset[si]
        st = sim_scene.Settings(sd["settings"], params.scene_scale_factor)
        for k in range(len(st.camera.start_positions)):
            runs.append((si, k))
    return runs


# the options of a test run that build_rollout / run_one / run_many take by keyword (None = off): the camera's, and the rollout's observers
CAMERA_OPTIONS = ("depth_noise", "depth_filter")
OBSERVER_OPTIONS = tuple(dict.fromkeys(block.option for block in record_blocks.BLOCKS))


def _known_options(who, options):
    """A name among `options` that is neither the camera's nor an observer's is a TypeError, as an unknown keyword is."""
    unknown = sorted(set(options) - set(CAMERA_OPTIONS + OBSERVER_OPTIONS))
    if unknown:
        raise TypeError(f"{who}() got an unexpected keyword argument {unknown[0]!r}")


def build_rollout(params, nbp, dataset, run, device, test_resolution=0.05, state=None, seed=0, grid=256, **options):
    """Scene + GT surface + camera + Rollout for one (scene, start pose) run (nbp_planning.py:414-492).  `options` (each None = off):
    the camera's `depth_noise` (the sensor model, utility/depth_noise.py) and `depth_filter` (the frame filter behind it,
    utility/depth_filter.py), and the rollout's observers `recon_metrics`, `view_metrics`, `fusion`, `surface_metrics`
    (Rollout.__init__)."""
    _known_options("build_rollout", options)
    si, k = run
    sd = dataset[si]
    settings = sim_scene.Settings(sd["settings"], params.scene_scale_factor)
    mesh = sim_scene.load_scene(os.path.join(dataset.data_path, sd["scene_name"], sd["obj_name"]),
                                params.scene_scale_factor, device)
    y_bins = sim_scene.y_bins_for(mesh.verts_host, 4)
    _, gt_dev = sim_scene.setup_gt_scene(params, settings, mesh, device, test_resolution, seed=seed)
    camera = setup_test_camera(params, mesh, settings.camera.start_positions[k], settings, device, seed=seed,
                               **{key: value for key, value in options.items() if key in CAMERA_OPTIONS})
    ro = Rollout(params, nbp, camera, gt_dev, mesh, mesh, y_bins, device, state, seed, grid,
                 **{key: value for key, value in options.items() if key in OBSERVER_OPTIONS})
    ro.scene_name, ro.start = sd["scene_name"], k
    return ro


def run_tags(policy_spec, noise_spec, filter_spec):
    """The entries that every record of a run carries for the options `policy`, `depth_noise` and `depth_filter`: those that are on
    (a normalised spec, not None), in that order, each a copy of its spec."""
    tags = {"policy": policy_spec, "depth_noise": noise_spec, "depth_filter": filter_spec}
    return {key: dict(spec) for key, spec in tags.items() if spec is not None}


def resolve_options(**given):
    """The planning options of a test run (_test_config's keys) as one record.  An option not given (or _UNSET) is the key of that
    name in the configs/test/ file load_params read last, None = off where that file has none; each then goes through its own
    make_policy / option_spec, in _test_config's order: a bad combination raises the first bad option's ValueError.  The record has
    the normalised spec (or None) under each option's name -- `policy` is the policy object, None = the network, with its options
    as `policy_spec`; `symmetry_ensemble` stays as given, checked here as its setter will -- and `rollout`, the keywords of
    build_rollout / run_one / run_many among them (`fusion` and `surface_metrics` only where they are on: off is those functions'
    default)."""
    from .frontier_policy import make_policy
    opts = SimpleNamespace()

    def ensemble(spec):
        if opts.policy is not None:
            opts.policy.symmetry_ensemble = spec           # (a policy refuses anything but None)
        else:
            augment.check_ensemble(spec)
        return spec

    normalise = {"policy": make_policy, "symmetry_ensemble": ensemble, "recon_metrics": recon_options.option_spec,
                 "depth_noise": noise_options.option_spec, "depth_filter": filter_options.option_spec,
                 "view_metrics": view_options.option_spec, "fusion": fusion_options.option_spec,
                 "surface_metrics": surface_options.option_spec}
    if set(given) - set(normalise):
        raise TypeError(f"resolve_options: unknown options {sorted(set(given) - set(normalise))}")
    for key in _test_config:
        value = given.get(key, _UNSET)
        value = _test_config[key] if value is _UNSET else value
        setattr(opts, key, normalise[key](None if value is _UNSET else value))
    opts.policy_spec = None if opts.policy is None else dict(opts.policy.options)
    opts.rollout = {key: getattr(opts, key) for key in ("recon_metrics", "depth_noise", "view_metrics", "depth_filter")}
    if opts.fusion is not None:
        opts.rollout["fusion"] = opts.fusion
    if opts.surface_metrics is not None:
        opts.rollout["surface_metrics"] = opts.surface_metrics
    return opts


def _result(ro, n_poses):
    res = {"scene": ro.scene_name, "start": ro.start, "coverage": ro.coverage_evolution(n_poses),
           "X_cam_history": ro.camera.X_cam_history.tolist(), "V_cam_history": ro.camera.V_cam_history.tolist(),
           "n_points": int(ro.st.cloud_count.item())}
    # the options `policy`, `depth_noise`, `depth_filter` that are on: the normalised specs the rollout was steered and its frames made with
    tags = run_tags(ro.nbp.options if _wants_maps(ro.nbp) else None, ro.camera.depth_noise, ro.camera.depth_filter)
    # the blocks of the observers that are on (record_blocks.ALL_BLOCKS), each measured once, at the rollout's end: the block, and the raw
    # sums and counts behind its ratios (what parallel_rollout's gathers carry); formed with what the rollout was made with.
    # `made` / `size` stand where collect_records has opts / params: a field that a Block.context of record_blocks.py starts
    # to read belongs here too (tests/test_record_blocks_host.py runs every context on both, on the CPU)
    made = SimpleNamespace(recon_metrics=ro.recon_spec, view_metrics=ro.view_spec, fusion=ro.fusion_spec, surface_metrics=ro.surface_spec)
    size = SimpleNamespace(image_height=ro.camera.image_height, image_width=ro.camera.image_width, zfar=ro.params.zfar,
                           sensor_range=ro.params.sensor_range)
    fused = None if ro.fusion is None else ro.fused_cloud()      # extracted once per record, however many blocks judge it

    def entries(block):
        raw = block.measure(ro, n_poses, fused)
        return {block.key: block.summarise(raw, *block.context(made, size, n_poses)), block.key + "_raw": raw.tolist()}

    return record_blocks.fill(res, record_blocks.blocks_on(made), entries, tags)


def _policy_or(nbp, policy):
    """The planning option `policy` (None / "nbp" = the network `nbp`; "frontier" / "infogain" or a dict of utility/frontier.py / infogain.py::option_spec; a
    policy object passes through) -> what the rollouts evaluate."""
    if _wants_maps(policy):
        return policy
    from .frontier_policy import make_policy
    return make_policy(policy) or nbp


def run_one(params, nbp, dataset, run, device, test_resolution=0.05, state=None, n_poses=N_POSES, seed=0, *, policy=None, **options):
    """`policy`: None = the network `nbp` (_policy_or); `options`: build_rollout's."""
    _known_options("run_one", options)
    nbp = _policy_or(nbp, policy)
    ro = build_rollout(params, nbp, dataset, run, device, test_resolution, state, seed, **options)
    nbp.eval()
    for _ in range(n_poses):
        ro.step()
    ro.finish()
    return _result(ro, n_poses)


def run_many(params, nbp, dataset, runs, device, seeds, test_resolution=0.05, n_poses=N_POSES, rollouts_per_gpu=48,
             grid=256, timing=None, *, policy=None, **options):
    """Runs `runs` in lock-step groups of `rollouts_per_gpu` (MultiRollout); same results as run_one each.  `timing` (a dict)
    receives the wall-clock seconds of scene / GT-surface / camera setup and of the stepping (device-synchronised).  `policy` and
    `options`: as in run_one."""
    import time
    out = []
    _known_options("run_many", options)
    nbp = _policy_or(nbp, policy)
    nbp.eval()
    for g0 in range(0, len(runs), rollouts_per_gpu):
        t0 = time.perf_counter()
        chunk = list(zip(runs[g0:g0 + rollouts_per_gpu], seeds[g0:g0 + rollouts_per_gpu]))
        ros = [build_rollout(params, nbp, dataset, run, device, test_resolution, None, seed, grid, **options) for run, seed in chunk]
        multi = MultiRollout(ros, nbp, device)
        if timing is not None:
            torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        for _ in range(n_poses):
            multi.step()
        multi.flush()
        out += [_result(ro, n_poses) for ro in ros]
        if timing is not None:
            torch.cuda.synchronize(device)
            timing["build_s"] = timing.get("build_s", 0.0) + (t1 - t0)
            timing["step_s"] = timing.get("step_s", 0.0) + (time.perf_counter() - t1)
        del ros, multi
        torch.cuda.empty_cache()
    return out


def collect_records(results, runs, mine, rank, world, device, opts, params, n_poses, scene_names):
    """The tail of a test run, behind run_many: all ranks call this with their own `results` (of the runs `mine` = shard(runs, rank,
    world), in that order) and the options record `opts` (resolve_options).  The coverage curves travel in gather_results, and the raw
    float64 numbers of every block that is on (record_blocks.ALL_BLOCKS) in a gather of their own each.  -> (gathered, out): every rank's
    list of gather_results, on rank 0 with each block formed from the gathered row in place of the locally formed one, on the other
    ranks without the blocks; and the dict that goes into the result JSON {scene name: {start: record}} (`scene_names`: by scene
    index), None off rank 0."""
    for run, res in zip(mine, results):
        res["run_id"] = runs.index(run)
    gathered = parallel_rollout.gather_results(results, runs, rank, world, device, n_poses)
    blocks = record_blocks.blocks_on(opts)
    for block in blocks:
        ctx = block.context(opts, params, n_poses)              # (from opts, params and n_poses alone: the same on every rank)
        if block.check is not None:
            for res in results:
                block.check(res, *ctx)
        formed = getattr(parallel_rollout, block.gather)(results, runs, rank, world, device, *ctx)      # {} off rank 0
        for r in gathered:
            r.pop(block.key, None)
            r.pop(block.key + "_raw", None)
            if rank == 0:
                r[block.key] = formed[r["run_id"]]
    if rank != 0:
        return gathered, None
    out = {}
    tags = run_tags(opts.policy_spec, opts.depth_noise, opts.depth_filter)
    for r in gathered:
        si, k = runs[r["run_id"]]
        rec = record_blocks.fill({"coverage": r["coverage"], "auc": r["auc"]}, blocks, lambda block: {block.key: r[block.key]},
                                 {key: dict(spec) for key, spec in tags.items()})
        for key in ("X_cam_history", "V_cam_history"):          # histories of other ranks stay in their part files
            if key in r:
                rec[key] = r[key]
        out.setdefault(scene_names[si], {})[str(k)] = rec
    return gathered, out


def test_nbp_planning(params_file, model_file, results_json_file, numGPU, test_scenes, test_resolution=0.05,
                      use_perfect_depth_map=False, compute_collision=False, load_json=False, dataset_path=None,
                      nbp_weights=None, configs_dir=None, results_dir=None, n_poses=N_POSES, seed=8, torch_seed=9,
                      rollouts_per_gpu=48, grid_size=256, nbp_precision=None, **options):
    """Same arguments as the reference (nbp_planning.py:364-374); `grid_size` / `nbp_precision` select
    BASELINE.json configs[4] (512 grid at the same 0.3125 units per pixel, bf16 convolutions).  `options`: the planning options
    (resolve_options; an unknown name is a TypeError).  Each is None = off, or what its option_spec takes; not given, it is the key of
    that name in the configs/test/ file load_params read last (absent there: off):
      `policy`             frontier_policy.make_policy (utility/frontier.py / infogain.py::option_spec): stands where the network does, "policy" in every record
      `symmetry_ensemble`  utility/augment.py::ENSEMBLES (a name, or a list of op codes): NBP.symmetry_ensemble of the loaded network
      `recon_metrics`      utility/recon_metrics.py::option_spec: "reconstruction", and with `curve` "reconstruction_curve", in every record
      `depth_noise`        utility/depth_noise.py::option_spec: the seeded sensor model behind the rasteriser, its spec in every record
      `depth_filter`       utility/depth_filter.py::option_spec: the frame filter behind the sensor, its spec in every record
      `view_metrics`       utility/view_metrics.py::option_spec: "views" in every record
      `fusion`             utility/tsdf.py::option_spec: a TSDF volume of every frame, "fusion" in every record (judged with `recon_metrics`' options, or its defaults); with `mesh` the fused triangle mesh too (utility/tsdf_mesh.py), "fusion_mesh" in every record (judged with `surface_metrics`' options, or its defaults)
      `surface_metrics`    utility/surface_metrics.py::option_spec: "surface" in every record
    With a policy no weights are loaded (`nbp_precision` given with it draws a warning).  Under torchrun the flattened (scene, start
    pose) runs are sharded round-robin over the ranks; the coverage curves are gathered with ONE all_gather over RCCL (backend
    "nccl" on ROCm; "gloo" on CPU-only hosts), and each record block that is on with one more (collect_records)."""
    import time
    from ..parallel_rollout import init_distributed, shard
    t_start = time.perf_counter()
    here = os.path.dirname(os.path.abspath(__file__))
    configs_dir = configs_dir or os.path.join(here, "../../configs/macarons")
    results_dir = results_dir or os.path.join(here, "../../data")
    params = load_params(os.path.join(configs_dir, params_file))
    params.test_scenes = test_scenes
    rank, world, local_rank = init_distributed()
    device = torch.device("cuda", local_rank if world > 1 else numGPU)
    torch.cuda.set_device(device)
    random.seed(seed); np.random.seed(seed); torch.manual_seed(torch_seed)
    opts = resolve_options(**options)
    nbp, policy_spec = opts.policy, opts.policy_spec
    assert nbp_precision in (None, "fp32", "fp32_split", "bf16"), nbp_precision
    if nbp is not None and nbp_precision is not None:
        import warnings
        warnings.warn(f"policy {policy_spec['name']!r} runs no network: nbp_precision={nbp_precision!r} has no effect "
                      "(nor have nbp_weights and model_file)", stacklevel=2)
    if nbp is None:
        nbp = NBP()
        if nbp_weights and os.path.exists(nbp_weights):
            ck = torch.load(nbp_weights, map_location="cpu")
            nbp.load_state_dict(ck["model_state_dict"])
        else:
            from ..utility.synthetic import make_explorer_state_dict
            print("[nbp] no checkpoint at", nbp_weights, "-> seeded synthetic weights")
            nbp.load_state_dict(make_explorer_state_dict(torch_seed))
        nbp.to(device).eval()
        if nbp_precision is not None:           # None: the model's default ("fp32_split")
            nbp.conv_precision = nbp_precision
    nbp.symmetry_ensemble = params.symmetry_ensemble = opts.symmetry_ensemble
    dataset = sim_scene.SceneDataset(dataset_path, test_scenes)
    runs = list_runs(dataset, params)
    mine = shard(runs, rank, world)
    timing = {"load_s": time.perf_counter() - t_start}          # parameters, weights (packed on first use), dataset listing
    with torch.no_grad():
        results = run_many(params, nbp, dataset, mine, device, [seed + 1000 * r[0] + r[1] for r in mine],
                           test_resolution, n_poses, rollouts_per_gpu, grid_size, timing=timing, **opts.rollout)
    t_gather = time.perf_counter()
    gathered, out = collect_records(results, runs, mine, rank, world, device, opts, params, n_poses,
                                    [dataset[si]["scene_name"] for si in range(len(dataset))])
    if rank == 0:
        os.makedirs(results_dir, exist_ok=True)
        with open(os.path.join(results_dir, results_json_file), "w") as fh:
            json.dump(out, fh)
        print("Saved data about test losses in", results_json_file)
        print("All trajectories computed.")
        # one machine-readable line for bench.py's full_rollout stage: where the wall clock of a whole test run goes
        timing.update(gather_write_s=time.perf_counter() - t_gather, total_s=time.perf_counter() - t_start, runs=len(runs),
                      runs_this_rank=len(mine), n_poses=n_poses, world=world, scenes=len(dataset))
        print("[nbp] timing " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in timing.items()}), flush=True)
    return gathered
