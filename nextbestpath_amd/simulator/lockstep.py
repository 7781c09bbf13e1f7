"""What the two lock-step drivers -- testers/nbp_planning.py::MultiRollout (exploration) and utility/nbp_utils.py::CollectionGroup
(training-data collection) -- share: the device-resident rollout state, the camera set-up, and ONE implementation of each group
stage that is the same in both (coverage and map arguments, un-projection of a group's frames, the render of a group's moves).
The host halves (replanning and heading draws there; experiences, hindsight relabelling, Boltzmann sampling and the commit order
here) differ and stay with their driver.  The only difference that crosses this boundary is "colours or not", as an argument.
Both drivers' set-up helpers live here too, so that neither imports the other: `setup_test_camera`, `_concurrent_streams` and
`_settle_gc` (with its NBP_GC_FREEZE read, the one use of `_lib`); testers/nbp_planning.py re-exports them under their old names.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..utility import hipops
from .camera import Camera

N_POSES = 101            # range(101) at nbp_planning.py:60
# frames of a step, as (offsets into the camera's newest frames, salt of the un-projection's sub-sampling seed)
CURRENT = ([-1], 0)
SUPERVISION = ([-5, -4, -3, -2], 5)
_GC_FREEZE = _lib.tune("NBP_GC_FREEZE", "1") == "1"


def _settle_gc():
    """A rollout's setup leaves ~10^5 long-lived Python objects behind (the lattice planner's node / edge tables); CPython's
    generational collector walks all of them in every full collection -- 70-80 ms, once or twice per 100-step rollout, i.e. as long
    as 80 exploration steps (tools/diag/single_step_spikes.py: 1140 steps/s with the collector off, 450-500 with it on over steps
    40-100).  After setup they are collected once and then FROZEN (gc.freeze: moved to the permanent generation, no longer walked;
    reference counting still frees them).  NBP_GC_FREEZE=0: off."""
    if _GC_FREEZE:
        import gc
        gc.collect()
        gc.freeze()


class RolloutState:
    """Device-resident rollout buffers (cloud, counters, per-step coverage counts)."""

    def __init__(self, device, capacity=3_400_000, grid=256):
        self.device = device
        self.cloud = torch.zeros(capacity, 3, dtype=torch.float32, device=device)
        self.cloud_rgb = torch.zeros(capacity, 3, dtype=torch.float32, device=device)        # full_pc_colors (ref :39)
        self.cloud_count = torch.zeros(1, dtype=torch.int64, device=device)
        self.coverage_counts = torch.zeros(N_POSES, 2, dtype=torch.int32, device=device)
        self.maps6 = torch.zeros(6, grid, grid, dtype=torch.float32, device=device)
        self.net_in = torch.zeros(1, 5, grid, grid, dtype=torch.float32, device=device)
        self.bins = None             # utils.CloudBins of `cloud` (made by the rollout: the tile grid needs the scene's extent)
        self.frames_appended = 0     # frames un-projected into the cloud so far (host bound of its size: <= that many x per-frame keep)
        self.frames_filed = 0        # ... of which the bins have seen (filed by the appending launch, or caught up by a two-launch build)
        self._overlap = None         # forward_overlap(): two network inputs / streams / event pairs, used alternately

    def forward_overlap(self):
        """Two network-input buffers with a forward stream and an event pair each (Rollout.step alternates between them, so that
        the forward of step t may still be reading its input while step t + 1 builds the next one)."""
        if self._overlap is None:
            main = torch.cuda.current_stream(self.device)
            ins = [self.net_in, torch.zeros_like(self.net_in)]
            # streams that really run beside `main` and beside each other (HIP maps streams onto four hardware queues; a forward
            # stream that shares main's queue serialises the step: 1100 -> 890 steps/s, seen in about one bench run in eight)
            streams, self.overlap_info = _concurrent_streams(self.device, len(ins), against=(main,))
            # (a high-priority third stream for the forward of a replanning step -- the one the step waits for, ahead of the dead
            # forwards still running beside it -- was measured: 1142 / 1157 against 1135 / 1138 steps/s, within noise; not kept)
            for f in streams:
                f.wait_stream(main)
            self._overlap = {"net_in": ins, "streams": streams, "maps": [torch.cuda.Event() for _ in ins],
                             "done": [torch.cuda.Event() for _ in ins], "used": [False for _ in ins]}
        return self._overlap


def _concurrent_streams(device, n, tries=24, cycles=300_000, against=(), priority=0):
    """n torch streams whose kernels the runtime really runs side by side, and how that was established.

    HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) when they are first used, and two streams on one
    queue run their kernels strictly one after the other -- the lock-step's two groups then stop overlapping.  Measured: after
    ANY hipGraph capture in the process (the single-rollout path's ForwardGraph) the next two pool streams land on one queue and
    the 48-rollout lock-step loses 6 % (profiles/r04/stream_queue_collision.txt).  So the streams are not taken on trust: a
    candidate is kept only if a short spin kernel on it overlaps with one on every stream already chosen (and on every stream of
    `against`: the single rollout's forward streams must run beside the stream the step itself is enqueued on)."""
    def overlap(a, b):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize(device)
        with torch.cuda.stream(a):
            ev[0].record()
            torch.cuda._sleep(cycles)
            ev[1].record()
        with torch.cuda.stream(b):
            torch.cuda._sleep(cycles)
            ev[2].record()
        torch.cuda.synchronize(device)
        return ev[0].elapsed_time(ev[2]) < 1.5 * ev[0].elapsed_time(ev[1])

    if not hasattr(torch.cuda, "_sleep"):          # (a torch without the spin kernel: the streams are taken as they come)
        return [torch.cuda.Stream(device, priority=priority) for _ in range(n)], {"streams_tested": 0, "concurrent": None}
    chosen, tested = [], 0
    while len(chosen) < n and tested < tries:
        st = torch.cuda.Stream(device, priority=priority)
        tested += 1
        with torch.cuda.stream(st):
            torch.cuda._sleep(1)                   # first use: the stream gets its hardware queue here
        if all(overlap(c, st) for c in list(against) + chosen):
            chosen.append(st)
    ok = len(chosen) == n
    while len(chosen) < n:                         # (never seen: fewer than n distinct queues among `tries` streams)
        chosen.append(torch.cuda.Stream(device, priority=priority))
    return chosen, {"streams_tested": tested, "concurrent": ok}


def setup_test_camera(params, mesh, start_cam_idx, settings, device, seed=0, depth_noise=None, depth_filter=None):
    """macarons/testers/scene.py:410-488: build the camera, step to the first collision-free
    neighbour of the start pose, capture, then walk to the start pose capturing 4 frames.  `depth_noise`: the camera's option of
    that name (None = off), set before these captures: they are frames 0..4 of its noise sequence.  `depth_filter`: the camera's
    option of that name (None = off): these captures pass through it too."""
    cam = Camera(settings.camera.x_min, settings.camera.x_max, settings.camera.pose_l, settings.camera.pose_w,
                 settings.camera.pose_h, settings.camera.pose_n_elev, settings.camera.pose_n_azim,
                 params.n_interpolation_steps, params.zfar, params.image_height, params.image_width, device,
                 params.gathering_factor, params.sensor_range, seed=seed,
                 ambient_light_intensity=getattr(params, "ambient_light_intensity", 0.85),
                 contrast_factor=getattr(settings.camera, "contrast_factor", 1.0), depth_noise=depth_noise,
                 depth_filter=depth_filter)
    start = tuple(int(v) for v in start_cam_idx)
    neigh = cam.get_neighboring_poses(start)
    segs = torch.from_numpy(np.stack([np.concatenate([cam.pose_from_idx(n)[:3], cam.pose_from_idx(start)[:3]])
                                      for n in neigh]).astype(np.float32)).to(device)
    hit = hipops.segments_hit_mesh(mesh.verts, mesh.faces, segs).cpu().numpy()
    free = [n for n, h in zip(neigh, hit) if not h]
    first = free[0] if free else neigh[0]          # the reference raises NameError when none is free
    cam.initialize_camera(first)
    cam.capture_image(mesh)
    cam.move_and_capture(mesh, start)
    return cam


class LockstepRollout:
    """The GPU stages of a step that exploration and collection rollouts have in common.  A subclass provides `params`, `st` (a
    RolloutState), `camera`, `mesh`, `y_bins`, `cov_plan`, `step_seed` (seed * 1_000_003: every draw of the step derives from it)
    and `pose_i` (the step's number)."""

    def coverage_item(self):
        """The coverage stage's arguments (hipops.coverage_count_batch / CoveragePlan.count): coverage of the cloud so far into row
        pose_i of the state's counts (a row is zero until its first use)."""
        st, pose_i = self.st, self.pose_i
        return (self.cov_plan, st.cloud, st.coverage_counts[pose_i % N_POSES], st.cloud_count, st.cloud.shape[0],
                self.step_seed + 7 * pose_i, pose_i < N_POSES)

    def count_coverage(self):
        plan, *args = self.coverage_item()
        return plan.count(*args)                   # (the item's order is CoveragePlan.count's)

    def recon_curve_item(self):
        """The per-step reconstruction curve's arguments (hipops.recon_curve_update_batch), or None where the rollout has no
        `recon_curve` (the planning option `recon_metrics` without `curve`): the cloud so far -- the one the coverage stage of this
        step saw -- into row pose_i of the curve.  The host bound of the new points counts the frames un-projected since the last
        item was made (making an item moves that mark: an item is made to be launched); it only sizes the grid."""
        curve = getattr(self, "recon_curve", None)
        if curve is None:
            return None
        st, params = self.st, self.params
        per_frame = int(params.image_height * params.image_width * params.gathering_factor) + 1
        new = st.frames_appended - self._curve_frames
        self._curve_frames = st.frames_appended
        return curve.item(st.cloud, st.cloud_count, self.pose_i % N_POSES, min(st.cloud.shape[0], new * per_frame))

    def update_recon_curve(self):
        item = self.recon_curve_item()
        if item is not None:
            hipops.recon_curve_update_batch([item])

    def unproject(self, frames, colours, clear=None):
        """Un-projects `frames` (CURRENT or SUPERVISION) of this rollout's camera into its cloud, with their colours when `colours`
        are wanted and the camera renders any.  While the state's bins are in step with the cloud (every frame so far filed, frames
        that the filing form takes) the launch files its points into them too, and zeroes `clear` = (maps6, trajectory channel) for
        the one-launch map build behind it (utils.step_maps(..., prefiled=True))."""
        which, salt = frames
        st, camera, params = self.st, self.camera, self.params
        depth, cams = camera.frames_batch(which)
        colour = camera.colour_source(which) if colours else {}
        filing = st.bins is not None and st.frames_filed == st.frames_appended and hipops.unproject_files(depth, None)
        hipops.unproject_append(depth, None, cams, st.cloud, st.cloud_count, params.gathering_factor, params.sensor_range,
                                seed=self.step_seed + 11 * self.pose_i + salt, cloud_rgb=st.cloud_rgb if colour else None,
                                bins=st.bins if filing else None, clear=clear if filing else None, **colour)
        st.frames_appended += len(which)
        if filing:
            st.frames_filed += len(which)
        fusion = getattr(self, "fusion", None)     # (option `fusion`: the same frames and cameras into the rollout's TSDF volume)
        if fusion is not None:
            fusion.integrate(depth, cams)

    def fusion_item(self, depth, cams):
        """The arguments of hipops.tsdf_integrate_batch for the frames this rollout un-projects (ring-slot pointers and their
        cameras), or None where the rollout has no `fusion` (the planning option of that name is off)."""
        fusion = getattr(self, "fusion", None)
        return None if fusion is None else fusion.item(depth, cams)

    def unproject_item(self, frames, colours):
        """Arguments of hipops.unproject_append_batch for `frames` of this rollout; None when its camera cannot take part in the
        batched call (Camera.ring_frames)."""
        which, salt = frames
        ring = self.camera.ring_frames(which, colours)
        if ring is None:
            return None
        depth, cams, shade = ring
        st = self.st
        return (self, depth, cams, st.cloud, st.cloud_count, self.step_seed + 11 * self.pose_i + salt, st.cloud_rgb if shade else None,
                shade)

    def maps_item(self):
        """The map stage's arguments (utils.step_maps / step_maps_batch) at the camera's current pose, which becomes `self.pose`:
        (cloud, host upper bound of its size, device size, pose, y_bins, trajectory history, n_old, fresh positions, bins | None).
        The bound counts the frames actually un-projected into the cloud (a frame keeps at most int(H W gathering_factor) pixels);
        it only sizes grids -- the kernels read the device count, and the binned build walks every page whatever the bound (ADVICE
        r03: a guessed bound must not drop points)."""
        st, params = self.st, self.params
        self.pose = self.camera.pose_from_idx(self.camera.cam_idx)
        traj_dev, n_old, fresh = self.camera.trajectory_pending()
        per_frame = int(params.image_height * params.image_width * params.gathering_factor) + 1
        return (st.cloud, min(st.cloud.shape[0], st.frames_appended * per_frame), st.cloud_count, self.pose, self.y_bins, traj_dev,
                n_old, fresh, st.bins)


def unproject_group(grp, frames, colours):
    """LockstepRollout.unproject for every rollout of a group: ONE batched call when every camera can take part in it, else one
    call per rollout (identical clouds either way)."""
    items = [r.unproject_item(frames, colours) for r in grp]
    if all(it is not None for it in items):
        p0, n = grp[0].params, len(frames[0])
        hipops.unproject_append_batch(items, p0.image_height, p0.image_width, n, p0.gathering_factor, p0.sensor_range)
        for r in grp:
            r.st.frames_appended += n
        # the option `fusion`: exactly these frames, with these cameras, into each rollout's TSDF volume, in ONE call (a launch per 12)
        fused = [f for f in (r.fusion_item(it[1], it[2]) for r, it in zip(grp, items)) if f is not None]
        if fused:
            hipops.tsdf_integrate_batch(fused, p0.image_height, p0.image_width)
    else:
        for r in grp:
            r.unproject(frames, colours)


def render_moves(grp, next_idx):
    """Every rollout of a group moves to its next lattice index (next_idx[i]): the 4 interpolated frames of all the moves are
    rendered in ONE rasteriser call when every camera defers its colours, else one call per rollout (identical frames).  Cameras
    with a sensor chain render into its first source slots (capture_begin hands those out); behind the render, stage kind by stage
    kind in chain order, ONE launch per spec over all the new frames of the cameras with that stage (a group shares one spec unless
    a caller mixes rollouts).  The same frames as alone: a frame's noise depends on its camera's seed, its id and the pixel only,
    its filtered value on that frame only."""
    p0 = grp[0].params
    moves = [r.camera.move_poses(idx) for r, idx in zip(grp, next_idx)]
    if not all(r.camera.deferred_colours(r.mesh) for r in grp):
        for r, cams in zip(grp, moves):
            r.camera.capture_images(r.mesh, cams)
        return
    pend = [r.camera.capture_begin(r.mesh, cams) for r, cams in zip(grp, moves)]
    hipops.raster_zface_batch([(r, r.mesh.verts, r.mesh.faces, cams, out, zf) for r, cams, (out, zf, _) in zip(grp, moves, pend)],
                              p0.image_height, p0.image_width, len(moves[0]))
    for kind, launch in {"noise": hipops.depth_noise_batch, "filter": hipops.depth_filter_batch}.items():
        by_spec = {}                               # spec key -> (spec, items), in first-appearance order
        for r, cams, (_, _, slot) in zip(grp, moves, pend):
            stage = r.camera.stages.get(kind)
            if stage is not None:
                by_spec.setdefault(stage.key, (stage.spec, []))[1].append(r.camera.stage_item(stage, slot, len(cams)))
        for spec, items in by_spec.values():
            launch(items, spec, p0.image_height, p0.image_width)
    for r, cams, (out, _, slot) in zip(grp, moves, pend):
        r.camera.capture_commit(out, cams, slot)
