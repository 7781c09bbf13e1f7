"""Thin tensor-level wrappers over the simulator / planner entry points of libnbp_hip.so
(pointers + sizes only; all arithmetic is in the HIP kernels).  Used by the rollout driver,
the reference-API mirrors and the GPU parity tests."""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from .. import _lib

TAN_HALF_FOV = float(torch.tensor(math.tan(math.radians(30.0)), dtype=torch.float32))   # FoV 60 deg (pytorch3d default)
Z_CLIP = 0.5                                                                            # znear / 2


def _st():
    return _lib.current_stream()


_ws = {}


def _workspace(tag, nbytes, device):
    # scratch is per (kind, device, STREAM): rollouts stepped on different streams run their kernels concurrently
    key = (tag, device.index if device.index is not None else -1, _st())
    w = _ws.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws[key] = w
    return w


_ws_sizes = {}


def _workspace_for(tag, size_key, size_fn, device):
    """Workspace whose size only depends on `size_key`: the C size query runs once per key."""
    n = _ws_sizes.get((tag, size_key))
    if n is None:
        n = _ws_sizes[(tag, size_key)] = int(size_fn())
    return _workspace(tag, n, device)


def cams12(R, T, device=None):
    """[n,3,3], [n,3] -> HOST numpy [n,12] fp32 (R row-major then T); cameras travel as kernel arguments."""
    import numpy as np
    R = np.asarray(R, np.float32).reshape(-1, 9)
    T = np.asarray(T, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([R, T], 1))


def _cam_arg(cams):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(cams, np.float32).reshape(-1, 12))
    return a, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0]


def unproject_files(depth, mask):
    """Can unproject_append(..., bins=) file this call's points?  (The filing rides on the three-launch form: H W % 4 == 0, 16-byte
    aligned frames.)"""
    F_, H, W = depth.shape
    return (H * W) % 4 == 0 and depth.data_ptr() % 16 == 0 and (mask is None or mask.data_ptr() % 4 == 0)


def unproject_append(depth, mask, cams, cloud, cloud_count, gathering_factor=0.05, fov_range=70.0, seed=0,
                     tan_half_fov=TAN_HALF_FOV, rgb=None, cloud_rgb=None, shade=None, bins=None, clear=None):
    """depth [F,H,W] fp32 (F <= 8), mask [F,H,W] uint8|None, cams host [F,12]; appends to cloud [cap,3] at the
    device counter cloud_count (int64[1]).  Returns counts [F,2] int32 (device): a VIEW into this stream's scratch, valid
    until the next unproject_append on the same stream -- clone it to keep it.
    bins (utils.CloudBins of `cloud`): the launch also files the appended points into the tile-binned store; clear = (maps6 [6,S,S],
    traj [S,S]): ... and zeroes what the map build behind it accumulates into (utils.step_maps(..., prefiled=True): one launch)."""
    F_, H, W = depth.shape
    if F_ > 8:
        raise ValueError("unproject_append: at most 8 frames per call")
    L = _lib.lib()
    keep, cam_ptr, _ = _cam_arg(cams)
    ws = _workspace_for("unproject", (F_, H, W), lambda: L.nbp_unproject_workspace_bytes(F_, H, W) + 256, depth.device)
    counts = ws[-64:].view(torch.int32).reshape(8, 2)[:F_]          # per-stream scratch: no allocation per call
    if bins is not None:
        zface = verts = faces = vcolors = None
        ambient = 0.85
        if shade is not None:
            zface, verts, faces, vcolors, ambient = shade
            rgb = None
        z6, z1, S = (None, None, 0) if clear is None else (clear[0], clear[1], int(clear[0].shape[-1]))
        rc = L.nbp_unproject_append_filed_f32(_lib.ptr(depth), _lib.ptr(mask), _lib.ptr(rgb), _lib.ptr(zface), _lib.ptr(verts),
                                              _lib.ptr(faces), _lib.ptr(vcolors), cam_ptr, F_, H, W, tan_half_fov, float(fov_range),
                                              float(gathering_factor), int(seed) & 0xFFFFFFFF, float(ambient), _lib.ptr(counts),
                                              _lib.ptr(cloud), _lib.ptr(cloud_rgb), _lib.ptr(cloud_count), cloud.shape[0],
                                              bins.store.data_ptr(), _lib.ptr(z6), _lib.ptr(z1), S, _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_unproject_append_filed_f32")
        return counts
    if shade is not None:      # deferred shading: (zface [F,H,W] int64, verts, faces, vcolors, ambient) -> colours of kept pixels
        zface, verts, faces, vcolors, ambient = shade
        rc = L.nbp_unproject_append_shaded_f32(_lib.ptr(depth), _lib.ptr(mask), _lib.ptr(zface), _lib.ptr(verts), _lib.ptr(faces),
                                               _lib.ptr(vcolors), cam_ptr, F_, H, W, tan_half_fov, float(fov_range),
                                               float(gathering_factor), int(seed) & 0xFFFFFFFF, float(ambient),
                                               _lib.ptr(counts), _lib.ptr(cloud), _lib.ptr(cloud_rgb), _lib.ptr(cloud_count),
                                               cloud.shape[0], _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_unproject_append_shaded_f32")
        return counts
    if rgb is not None:        # colours of the kept pixels ride along (compute_partial_point_cloud with images)
        rc = L.nbp_unproject_append_rgb_f32(_lib.ptr(depth), _lib.ptr(mask), _lib.ptr(rgb), cam_ptr, F_, H, W, tan_half_fov,
                                            float(fov_range), float(gathering_factor), int(seed) & 0xFFFFFFFF,
                                            _lib.ptr(counts), _lib.ptr(cloud), _lib.ptr(cloud_rgb), _lib.ptr(cloud_count),
                                            cloud.shape[0], _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_unproject_append_rgb_f32")
        return counts
    rc = L.nbp_unproject_append_f32(_lib.ptr(depth), _lib.ptr(mask), cam_ptr, F_, H, W, tan_half_fov,
                                    float(fov_range), float(gathering_factor), int(seed) & 0xFFFFFFFF,
                                    _lib.ptr(counts), _lib.ptr(cloud), _lib.ptr(cloud_count), cloud.shape[0],
                                    _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_unproject_append_f32")
    return counts


def raster_zbuf(verts, faces, cams, H, W, bin_cap=2048, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP, out=None,
                overflow=None):
    """verts [V,3] fp32, faces [F,3] int32, cams host [n,12] -> zbuf [n,H,W] (-1 background)."""
    L = _lib.lib()
    keep, cam_ptr, n = _cam_arg(cams)
    if out is None:
        out = torch.empty(n, H, W, dtype=torch.float32, device=verts.device)
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=verts.device)
    nf = faces.shape[0]
    ws = _workspace_for("raster", (nf, n, H, W), lambda: L.nbp_raster_workspace_bytes(nf, n, H, W, bin_cap), verts.device)
    rc = L.nbp_raster_zbuf_f32(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], cam_ptr, n, H,
                               W, tan_half_fov, z_clip, bin_cap, _lib.ptr(out), _lib.ptr(overflow), _lib.ptr(ws),
                               ws.numel(), _st())
    _lib.check(rc, "nbp_raster_zbuf_f32")
    return out, overflow


def raster_rgbz(verts, faces, vcolors, cams, H, W, ambient=0.85, contrast=1.0, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP,
                out_z=None, out_rgb=None):
    """Camera.capture_image with colours -> (zbuf [n,H,W], rgb [n,H,W,3])."""
    L = _lib.lib()
    keep, cam_ptr, n = _cam_arg(cams)
    if out_z is None:
        out_z = torch.empty(n, H, W, dtype=torch.float32, device=verts.device)
    if out_rgb is None:
        out_rgb = torch.empty(n, H, W, 3, dtype=torch.float32, device=verts.device)
    nf = faces.shape[0]
    ws = _workspace_for("raster_rgb", (nf, n, H, W), lambda: L.nbp_raster_rgb_workspace_bytes(nf, n, H, W), verts.device)
    rc = L.nbp_raster_rgbz_f32(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), nf, _lib.ptr(vcolors), cam_ptr, n, H, W,
                               tan_half_fov, z_clip, float(ambient), float(contrast), _lib.ptr(out_z), _lib.ptr(out_rgb),
                               _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_raster_rgbz_f32")
    return out_z, out_rgb


def raster_zface(verts, faces, cams, H, W, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP, out_z=None, out_zface=None):
    """Depth render that also returns zface [n,H,W] int64 = (depth bits << 32 | nearest face), -1 for background: the
    input of the deferred colour evaluation (shade_image / unproject_append(shade=...))."""
    L = _lib.lib()
    keep, cam_ptr, n = _cam_arg(cams)
    if out_z is None:
        out_z = torch.empty(n, H, W, dtype=torch.float32, device=verts.device)
    if out_zface is None:
        out_zface = torch.empty(n, H, W, dtype=torch.int64, device=verts.device)
    nf = faces.shape[0]
    ws = _workspace_for("raster", (nf, n, H, W), lambda: L.nbp_raster_workspace_bytes(nf, n, H, W, 0), verts.device)
    rc = L.nbp_raster_zface_f32(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), nf, cam_ptr, n, H, W, tan_half_fov, z_clip,
                                _lib.ptr(out_z), _lib.ptr(out_zface), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_raster_zface_f32")
    return out_z, out_zface


def shade_image(zface, verts, faces, vcolors, cams, ambient=0.85, tan_half_fov=TAN_HALF_FOV, out=None):
    """rgb [n,H,W,3] of frames rendered by raster_zface (bit-identical to raster_rgbz with contrast 1)."""
    L = _lib.lib()
    keep, cam_ptr, n = _cam_arg(cams)
    _, H, W = zface.shape
    if out is None:
        out = torch.empty(n, H, W, 3, dtype=torch.float32, device=verts.device)
    rc = L.nbp_shade_image_f32(_lib.ptr(zface), _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(vcolors), cam_ptr, n, H, W,
                               tan_half_fov, float(ambient), 1.0, _lib.ptr(out), _st())
    _lib.check(rc, "nbp_shade_image_f32")
    return out


def segments_hit_mesh(verts, faces, segs):
    """segs [E,6] fp32 device -> int32 [E] (1 = the segment hits the mesh)."""
    hit = torch.empty(segs.shape[0], dtype=torch.int32, device=verts.device)
    rc = _lib.lib().nbp_segments_hit_mesh_f32(_lib.ptr(verts), _lib.ptr(faces), faces.shape[0], _lib.ptr(segs),
                                              segs.shape[0], _lib.ptr(hit), _st())
    _lib.check(rc, "nbp_segments_hit_mesh_f32")
    return hit


def axis_ray_counts(verts, faces, pts):
    cnt = torch.empty(pts.shape[0], 3, dtype=torch.int32, device=verts.device)
    rc = _lib.lib().nbp_axis_ray_counts_f32(_lib.ptr(verts), _lib.ptr(faces), faces.shape[0], _lib.ptr(pts),
                                            pts.shape[0], _lib.ptr(cnt), _st())
    _lib.check(rc, "nbp_axis_ray_counts_f32")
    return cnt


def slice_obstacle(verts, faces, y0, cx, cz, S=256, grid_range=(-40, 40), half_width_px=1.04, out=None):
    """GT obstacle label [S,S] fp32 {0,1} around (cx, cz) at height y0 (ref utils.py:226-262)."""
    if out is None:
        out = torch.empty(S, S, dtype=torch.float32, device=verts.device)
    rc = _lib.lib().nbp_slice_obstacle_f32(_lib.ptr(verts), _lib.ptr(faces), faces.shape[0], float(y0), float(cx), float(cz),
                                           S, float(grid_range[0]), float(grid_range[1]), float(half_width_px),
                                           _lib.ptr(out), _st())
    _lib.check(rc, "nbp_slice_obstacle_f32")
    return out


def reference_figure_geometry(S=256, view_size=80.0):
    """(half_u, scale_u, half_v, scale_v, half_width_px, cap_px) of the reference's label image (utils.py:232-258): a 2.56 in figure
    at 100 dpi whose default axes box is 0.775 x 0.77 of it (198.4 x 197.12 px), x limits view_size wide, y limits shrunk to the box's
    aspect, the box saved as 198 x 197 px ('tight' bbox, pad 0), resized to S x S, flipped left-right; lines 1.5 pt wide with
    projecting caps.  Pinned by tests/golden/obstacle_label.npz."""
    fig = 2.56 * 100.0
    ax_w, ax_h = 0.775 * fig, 0.77 * fig                   # matplotlib's default subplot box: left .125 right .9 bottom .11 top .88
    png_w, png_h = int(ax_w), int(ax_h)                    # the saved crop
    px_per_unit = ax_w / view_size                         # equal aspect: the same on both axes before the resize
    scale_u, scale_v = px_per_unit * S / png_w, px_per_unit * S / png_h
    centre_u = S - (ax_w / 2.0) * S / png_w                # after the left-right flip
    centre_v = (png_h - ax_h / 2.0) * S / png_h            # rows count from the top of the 197-px crop
    half_width = 0.5 * (1.5 * 100.0 / 72.0) * 0.5 * (S / png_w + S / png_h)
    return centre_u / scale_u, scale_u, centre_v / scale_v, scale_v, half_width, half_width


def slice_obstacle_fig(verts, faces, y0, cx, cz, S=256, view_size=80.0, out=None):
    """The GT obstacle label on the reference's own pixel grid (nbp_slice_obstacle_fig_f32)."""
    if out is None:
        out = torch.empty(S, S, dtype=torch.float32, device=verts.device)
    hu, su, hv, sv, hw, cap = reference_figure_geometry(S, view_size)
    rc = _lib.lib().nbp_slice_obstacle_fig_f32(_lib.ptr(verts), _lib.ptr(faces), faces.shape[0], float(y0), float(cx), float(cz),
                                               S, hu, su, hv, sv, hw, cap, _lib.ptr(out), _st())
    _lib.check(rc, "nbp_slice_obstacle_fig_f32")
    return out


def slice_obstacle_fig_batch(items, S=256, view_size=80.0, out=None):
    """slice_obstacle_fig for several poses in one launch (nbp_slice_obstacle_fig_batch_f32): items = [(verts, faces, y0, cx, cz)],
    each its own mesh -> out [n,S,S] fp32 (bit-identical to n single calls).  More than 16 items go in chunks of 16."""
    import numpy as np
    n = len(items)
    if out is None:
        out = torch.empty(n, S, S, dtype=torch.float32, device=items[0][0].device)
    if n > 16:
        for i in range(0, n, 16):
            slice_obstacle_fig_batch(items[i:i + 16], S, view_size, out[i:i + 16])
        return out
    if tuple(out.shape) != (n, S, S) or not out.is_contiguous():
        raise ValueError("slice_obstacle_fig_batch: a contiguous out [n,S,S] expected")
    VP, I = C.c_void_p, C.c_int
    ve, fa, nf = (VP * max(n, 1))(), (VP * max(n, 1))(), (I * max(n, 1))()
    pose = np.zeros((max(n, 1), 3), np.float32)
    for i, (verts, faces, y0, cx, cz) in enumerate(items):
        ve[i], fa[i], nf[i] = verts.data_ptr(), faces.data_ptr(), faces.shape[0]
        pose[i] = (y0, cx, cz)
    hu, su, hv, sv, hw, cap = reference_figure_geometry(S, view_size)
    rc = _lib.lib().nbp_slice_obstacle_fig_batch_f32(n, ve, fa, nf, pose.ctypes.data, S, hu, su, hv, sv, hw, cap,
                                                     _lib.ptr(out) if n else None, _st())
    _lib.check(rc, "nbp_slice_obstacle_fig_batch_f32")
    return out


def goal_values_batch(items, V, grid_range=(-40, 40)):
    """Boltzmann goal scores for the rollouts of a group that replan (nbp_goal_values_batch_f32, one launch per 16): items =
    [(pos [P,3] device, (cx, cz), out1 [8,V,V] device, cell out [P] int32, val out [P] fp32)]; cell = row * V + col, -1 outside
    the window; val = out1.amax(0) at the clamped cell."""
    import numpy as np
    if len(items) > 16:
        for i in range(0, len(items), 16):
            goal_values_batch(items[i:i + 16], V, grid_range)
        return
    n = len(items)
    VP, I = C.c_void_p, C.c_int
    pos, npos, o1, cell, val = (VP * n)(), (I * n)(), (VP * n)(), (VP * n)(), (VP * n)()
    cxcz = np.zeros((n, 2), np.float32)
    for i, (p, (cx, cz), out1, c, v) in enumerate(items):
        if not (out1.is_contiguous() and c.is_contiguous() and v.is_contiguous() and p.is_contiguous()):
            raise ValueError("goal_values_batch: contiguous tensors expected")
        pos[i], npos[i], o1[i], cell[i], val[i] = p.data_ptr(), p.shape[0], out1.data_ptr(), c.data_ptr(), v.data_ptr()
        cxcz[i] = (cx, cz)
    rc = _lib.lib().nbp_goal_values_batch_f32(n, pos, npos, cxcz.ctypes.data, o1, int(V), float(grid_range[0]), float(grid_range[1]),
                                              cell, val, _st())
    _lib.check(rc, "nbp_goal_values_batch_f32")


def hindsight_cells_batch(items, V, grid_range=(-40, 40)):
    """Hindsight relabelling cells (nbp_hindsight_cells_batch_i32, one launch per 16): items = [(xz [m,2] fp32 device, cells out
    [m,m] int32)]; cells[i, j] = row * V + col of pose j in the frame of pose i (j > i, inside the window), else -1."""
    if len(items) > 16:
        for i in range(0, len(items), 16):
            hindsight_cells_batch(items[i:i + 16], V, grid_range)
        return
    n = len(items)
    VP, I = C.c_void_p, C.c_int
    xz, m, cells = (VP * n)(), (I * n)(), (VP * n)()
    for i, (p, c) in enumerate(items):
        if not (p.is_contiguous() and c.is_contiguous()) or c.numel() != p.shape[0] ** 2:
            raise ValueError("hindsight_cells_batch: contiguous xz [m,2] and cells [m,m] expected")
        xz[i], m[i], cells[i] = p.data_ptr(), p.shape[0], c.data_ptr()
    rc = _lib.lib().nbp_hindsight_cells_batch_i32(n, xz, m, int(V), float(grid_range[0]), float(grid_range[1]), cells, _st())
    _lib.check(rc, "nbp_hindsight_cells_batch_i32")


def fuse_obstacle(out2, maps6, traj, threshold=0.13):
    S = maps6.shape[-1]
    obst = torch.empty(S, S, dtype=torch.float32, device=maps6.device)
    fullproj = torch.empty(S, S, dtype=torch.float32, device=maps6.device)
    rc = _lib.lib().nbp_fuse_obstacle_f32(_lib.ptr(out2), _lib.ptr(maps6), _lib.ptr(traj), float(threshold), S,
                                          _lib.ptr(obst), _lib.ptr(fullproj), _st())
    _lib.check(rc, "nbp_fuse_obstacle_f32")
    return obst, fullproj


def score_candidates(pos, pose_xyz, out1, fullproj, skip=None, grid_range=(-40, 40)):
    """pos [P,3] device; out1 [8,V,V] device; -> (valid u8 [P], cell int32 [P,2], score f64 [P]) on device."""
    P, V, S = pos.shape[0], out1.shape[-1], fullproj.shape[-1]
    dev = pos.device
    valid = torch.empty(P, dtype=torch.uint8, device=dev)
    cell = torch.empty(P, 2, dtype=torch.int32, device=dev)
    score = torch.empty(P, dtype=torch.float64, device=dev)
    rc = _lib.lib().nbp_score_candidates_f32(_lib.ptr(pos), P, float(pose_xyz[0]), float(pose_xyz[2]), _lib.ptr(out1),
                                             V, _lib.ptr(fullproj), S, float(grid_range[0]), float(grid_range[1]),
                                             _lib.ptr(skip), _lib.ptr(valid), _lib.ptr(cell), _lib.ptr(score), _st())
    _lib.check(rc, "nbp_score_candidates_f32")
    return valid, cell, score


def edges_blocked(obst, pose_xyz, pos, edges, grid_range=(-40, 40)):
    E = edges.shape[0]
    out = torch.empty(E, dtype=torch.uint8, device=pos.device)
    rc = _lib.lib().nbp_edges_blocked_u8(_lib.ptr(obst), obst.shape[-1], float(grid_range[0]), float(grid_range[1]),
                                         float(pose_xyz[0]), float(pose_xyz[2]), _lib.ptr(pos), _lib.ptr(edges), E,
                                         _lib.ptr(out), _st())
    _lib.check(rc, "nbp_edges_blocked_u8")
    return out


def coverage_count(gt, pc, n_dev=None, n=None, weight=2, seed=0, threshold=1.0, bbox=None, out=None):
    """-> (count int32[1], m int32[1]) device tensors; coverage = count / len(gt)."""
    L = _lib.lib()
    G = gt.shape[0]
    k = int(G * weight)
    if bbox is None:
        lo, hi = gt.min(0).values.tolist(), gt.max(0).values.tolist()
    else:
        lo, hi = bbox
    lo_a, hi_a = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
    ws = _workspace("coverage", L.nbp_coverage_workspace_bytes(lo_a, hi_a, float(threshold), k), gt.device)
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=gt.device)
    N = pc.shape[0] if n is None else int(n)
    rc = L.nbp_coverage_count_f32(_lib.ptr(gt), G, _lib.ptr(pc), N, _lib.ptr(n_dev), k, int(seed) & 0xFFFFFFFF,
                                  float(threshold), lo_a, hi_a, out[0:1].data_ptr(), out[1:2].data_ptr(), _lib.ptr(ws),
                                  ws.numel(), _st())
    _lib.check(rc, "nbp_coverage_count_f32")
    return out


class CoveragePlan:
    """GT cloud sorted once into the coverage grid (one per rollout); `count` then costs one kernel per call."""

    def __init__(self, gt, threshold=1.0, weight=2, bbox=None):
        L = _lib.lib()
        self.gt, self.G, self.thr, self.k = gt, gt.shape[0], float(threshold), int(gt.shape[0] * weight)
        lo, hi = (gt.min(0).values.tolist(), gt.max(0).values.tolist()) if bbox is None else bbox
        self.lo, self.hi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
        self.plan = torch.empty(L.nbp_coverage_plan_bytes(self.lo, self.hi, self.thr, self.G), dtype=torch.uint8,
                                device=gt.device)
        ws = torch.empty(L.nbp_coverage_plan_workspace_bytes(self.lo, self.hi, self.thr, self.G), dtype=torch.uint8,
                         device=gt.device)
        rc = L.nbp_coverage_plan_build_f32(_lib.ptr(gt), self.G, self.thr, self.lo, self.hi, _lib.ptr(self.plan),
                                           self.plan.numel(), _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_coverage_plan_build_f32")
        self.epoch = 0
        self._m = torch.zeros(1, dtype=torch.int32, device=gt.device)

    def count(self, pc, out, n_dev=None, n=None, seed=0, out_is_zero=False):
        """Adds the covered-GT count to out[0] (int32 device; zeroed first unless out_is_zero), out[1] = sample size."""
        if not out_is_zero:
            out[0:1].zero_()
        self.epoch += 1
        N = pc.shape[0] if n is None else int(n)
        rc = _lib.lib().nbp_coverage_count_planned_f32(_lib.ptr(self.plan), self.G, self.thr, self.lo, self.hi, _lib.ptr(pc), N,
                                                       _lib.ptr(n_dev), self.k, int(seed) & 0xFFFFFFFF, self.epoch,
                                                       out[0:1].data_ptr(), out[1:2].data_ptr(), _st())
        _lib.check(rc, "nbp_coverage_count_planned_f32")
        return out


def replan_batch(items, S, V, grid_range=(-40, 40), threshold=0.13):
    """fuse_obstacle + score_candidates + edges_blocked for several rollouts in two launches; items = one tuple per
    rollout from LatticePlanner.replan_item.  More than 16 items go in chunks of 16."""
    import numpy as np
    if len(items) > 16:
        for i in range(0, len(items), 16):
            replan_batch(items[i:i + 16], S, V, grid_range, threshold)
        return
    n = len(items)
    VP, I = C.c_void_p, C.c_int
    a = [(VP * n)() for _ in range(13)]
    P, E = (I * n)(), (I * n)()
    xz = np.zeros((n, 2), np.float32)
    for i, (out2, maps6, traj, obst, fullproj, pos, cxz, out1, skip, valid, cell, score, edges, blocked) in enumerate(items):
        for arr, t in zip(a, (out2, maps6, traj, obst, fullproj, pos, out1, skip, valid, cell, score, edges, blocked)):
            arr[i] = None if t is None else t.data_ptr()
        P[i], E[i] = pos.shape[0], edges.shape[0]
        xz[i] = cxz
    o2, m6, tr, ob, fp, ps, o1, sk, va, ce, sc, ed, bl = a
    rc = _lib.lib().nbp_replan_batch_f32(n, o2, m6, tr, float(threshold), int(S), ob, fp, ps, P, xz.ctypes.data, o1, int(V),
                                         float(grid_range[0]), float(grid_range[1]), sk, va, ce, sc, ed, E, bl, _st())
    _lib.check(rc, "nbp_replan_batch_f32")


def coverage_count_batch(items):
    """CoveragePlan.count for several rollouts in two launches: items = [(plan, pc, out[2] int32, n_dev, n, seed, out_is_zero)]
    (more than 16 go in chunks of 16); the plans share the threshold."""
    import numpy as np
    if len(items) > 16:
        for i in range(0, len(items), 16):
            coverage_count_batch(items[i:i + 16])
        return
    n = len(items)
    VP, LL, U, I = C.c_void_p, C.c_longlong, C.c_uint, C.c_int
    plans, G, pc, N, ndev, k, seed, epoch, cnt, mout = (VP * n)(), (I * n)(), (VP * n)(), (LL * n)(), (VP * n)(), (LL * n)(), (U * n)(), \
        (U * n)(), (VP * n)(), (VP * n)()
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i, (plan, cloud, out, n_dev, nn, sd, out_is_zero) in enumerate(items):
        if not out_is_zero:
            out[0:1].zero_()
        plan.epoch += 1
        plans[i], G[i], pc[i], N[i] = plan.plan.data_ptr(), plan.G, cloud.data_ptr(), cloud.shape[0] if nn is None else int(nn)
        ndev[i], k[i], seed[i], epoch[i] = _lib.ptr(n_dev), plan.k, int(sd) & 0xFFFFFFFF, plan.epoch
        cnt[i], mout[i] = out[0:1].data_ptr(), out[1:2].data_ptr()
        lo[i], hi[i] = list(plan.lo), list(plan.hi)
    rc = _lib.lib().nbp_coverage_count_planned_batch_f32(n, plans, G, items[0][0].thr, lo.ctypes.data, hi.ctypes.data, pc, N, ndev, k, seed,
                                                         epoch, cnt, mout, _st())
    _lib.check(rc, "nbp_coverage_count_planned_batch_f32")


def _item_ws(tag, owner, key, nbytes, device):
    """Per-item scratch of the batched stages (items run concurrently: no sharing between rollouts).  The scratch belongs to
    `owner` (the rollout: any object with a __dict__) and is released with it -- a module-level cache keyed by id(rollout) kept
    ~1.2 KB per face per rollout alive for the life of the process."""
    store = owner.__dict__.setdefault("_hip_scratch", {})
    w = store.get((tag, key))
    if w is None or w.numel() < nbytes:
        w = store[(tag, key)] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return w


def unproject_append_batch(items, H, W, n_frames, gathering_factor=0.05, fov_range=70.0, tan_half_fov=TAN_HALF_FOV):
    """unproject_append for several rollouts in three launches.  items = [(key, depth frames [F tensors [H,W]], cams host
    [F,12], cloud, cloud_count, seed, cloud_rgb | None, shade | None)] with shade = (zface frames [F tensors [H,W] int64], verts,
    faces, vcolors, ambient); the frames need not be adjacent in memory; `key` is the rollout OBJECT: it owns its scratch.
    More than 12 items go in chunks of 12.  The coloured items of a call share ONE ambient: different values raise ValueError
    before anything is launched, in whichever chunks they fall."""
    import numpy as np
    # ONE ambient reaches the kernel: the coloured items must agree on it (checked on the whole list, before the chunking)
    ambients = {float(it[7][4]) for it in items if it[7] is not None and it[6] is not None}
    if len(ambients) > 1:
        raise ValueError(f"unproject_append_batch: the coloured items of one call carry different ambient values {sorted(ambients)}")
    if len(items) > 12:
        for i in range(0, len(items), 12):
            unproject_append_batch(items[i:i + 12], H, W, n_frames, gathering_factor, fov_range, tan_half_fov)
        return
    n = len(items)
    L = _lib.lib()
    VP, LL, U = C.c_void_p, C.c_longlong, C.c_uint
    wsb = int(L.nbp_unproject_workspace_bytes(n_frames, H, W)) + 512
    dep, zf = (VP * (n * n_frames))(), (VP * (n * n_frames))()
    ve, fa, vc, cnts, cl, crgb, ccount, cap, wsp, seeds = (VP * n)(), (VP * n)(), (VP * n)(), (VP * n)(), (VP * n)(), (VP * n)(), (VP * n)(), \
        (LL * n)(), (VP * n)(), (U * n)()
    cams = np.zeros((n, n_frames, 12), np.float32)
    ambient = ambients.pop() if ambients else 0.85
    for i, (key, depth, cam, cloud, cloud_count, seed, cloud_rgb, shade) in enumerate(items):
        ws = _item_ws("unproject", key, (n_frames, H, W), wsb, cloud.device)
        cl[i], ccount[i], cap[i], wsp[i], seeds[i] = cloud.data_ptr(), cloud_count.data_ptr(), cloud.shape[0], ws.data_ptr(), \
            int(seed) & 0xFFFFFFFF
        cnts[i] = ws.data_ptr() + wsb - 256               # 2 n_frames ints in the tail of the item's scratch
        cams[i] = np.asarray(cam, np.float32).reshape(n_frames, 12)
        for f in range(n_frames):
            dep[i * n_frames + f] = depth[f] if isinstance(depth[f], int) else depth[f].data_ptr()
        if shade is not None and cloud_rgb is not None:
            zface, verts, faces, vcolors, _ = shade
            for f in range(n_frames):
                zf[i * n_frames + f] = zface[f] if isinstance(zface[f], int) else zface[f].data_ptr()
            ve[i], fa[i], vc[i], crgb[i] = verts.data_ptr(), faces.data_ptr(), vcolors.data_ptr(), cloud_rgb.data_ptr()
    rc = L.nbp_unproject_append_shaded_batch_f32(n, dep, zf, ve, fa, vc, cams.ctypes.data, n_frames, H, W, tan_half_fov, float(fov_range),
                                                 float(gathering_factor), seeds, float(ambient), cnts, cl, crgb, ccount, cap, wsp,
                                                 wsb - 256, _st())
    _lib.check(rc, "nbp_unproject_append_shaded_batch_f32")


def raster_zface_batch(items, H, W, n_frames, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """raster_zface for several rollouts, each its own mesh, in four launches.  items = [(key = the rollout object, which owns the
    scratch, verts, faces, cams host [F,12], out_z [F,H,W], out_zface [F,H,W] int64)].  More than 12 items go in chunks of 12."""
    import numpy as np
    if len(items) > 12:
        for i in range(0, len(items), 12):
            raster_zface_batch(items[i:i + 12], H, W, n_frames, tan_half_fov, z_clip)
        return
    n = len(items)
    L = _lib.lib()
    VP, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    ve, nv, fa, nf, zb, zf, wsp, wsn = (VP * n)(), (I * n)(), (VP * n)(), (I * n)(), (VP * n)(), (VP * n)(), (VP * n)(), (SZ * n)()
    cams = np.zeros((n, n_frames, 12), np.float32)
    for i, (key, verts, faces, cam, out_z, out_zface) in enumerate(items):
        F_ = faces.shape[0]
        nb = _ws_sizes.get(("raster", (F_, n_frames, H, W)))
        if nb is None:
            nb = _ws_sizes[("raster", (F_, n_frames, H, W))] = int(L.nbp_raster_workspace_bytes(F_, n_frames, H, W, 0))
        ws = _item_ws("raster", key, (F_, n_frames, H, W), nb, verts.device)
        ve[i], nv[i], fa[i], nf[i], zb[i], zf[i], wsp[i], wsn[i] = verts.data_ptr(), verts.shape[0], faces.data_ptr(), F_, out_z.data_ptr(), \
            out_zface.data_ptr(), ws.data_ptr(), ws.numel()
        cams[i] = np.asarray(cam, np.float32).reshape(n_frames, 12)
    rc = L.nbp_raster_zface_batch_f32(n, ve, nv, fa, nf, cams.ctypes.data, n_frames, H, W, tan_half_fov, z_clip, zb, zf, wsp, wsn, _st())
    _lib.check(rc, "nbp_raster_zface_batch_f32")


def _frame_pointers(who, what, items, H, W):
    """The frame lists of a batched sensor launch's items, checked -> (source pointers, output pointers, H, W), frame by frame.
    items = [(source frames, output frames, per-frame ids | None)]: 1 to 4 frames per item, lists of one length, each frame a
    contiguous fp32 [H,W] tensor of the one shape or a device pointer (then H and W are needed).  `who` names the caller in the
    messages, `what` its source frames."""
    src, dst = [], []
    for fr, out, ids in items:
        if not (1 <= len(fr) <= 4 and len(out) == len(fr) and (ids is None or len(ids) == len(fr))):
            raise ValueError(f"{who}: an item has 1 to 4 {what} frames and as many output frames" + (" and frame ids" if ids is not None else ""))
        for t in (t for pair in zip(fr, out) for t in pair):
            if not isinstance(t, int):
                if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or (H is not None and tuple(t.shape) != (H, W)):
                    raise ValueError(f"{who}: frames are contiguous fp32 [H,W] tensors of one shape")
                H, W = t.shape
        src += [t if isinstance(t, int) else t.data_ptr() for t in fr]
        dst += [t if isinstance(t, int) else t.data_ptr() for t in out]
    if src and (H is None or W is None):
        raise ValueError(f"{who}: frames given as pointers need H and W")
    return src, dst, H, W


# ---- the depth-sensor noise model (csrc/nbp_depth_noise.hip; the definition is utility/depth_noise.py)
def _noise_args(spec):
    from . import depth_noise as dn
    spec = dn.option_spec(spec)
    if spec is None:
        raise ValueError("depth_noise: a spec is needed (None means off: nothing to launch)")
    return (spec["sigma_base"], spec["sigma_quad"], spec["z_min"], dn.dropout_threshold(spec["dropout"]), spec["edge_threshold"])


def depth_noise(clean, out, seed, first_frame, spec):
    """The noise model on clean [n,H,W] (or [H,W]) fp32 -> out (same shape, another buffer): frame i of one camera with word seed
    `seed` and frame id first_frame + i (mod 2^32); spec: depth_noise.option_spec's dict.  One launch.  Returns out."""
    if clean.dtype != torch.float32 or out.dtype != torch.float32 or clean.shape != out.shape or clean.dim() not in (2, 3):
        raise ValueError("depth_noise: clean and out are fp32 [n,H,W] (or [H,W]) of one shape")
    n = clean.shape[0] if clean.dim() == 3 else 1
    H, W = clean.shape[-2:]
    rc = _lib.lib().nbp_depth_noise_f32(_lib.ptr(clean), _lib.ptr(out), n, H, W, int(seed) & 0xFFFFFFFF, int(first_frame) & 0xFFFFFFFF,
                                        *_noise_args(spec), _st())
    _lib.check(rc, "nbp_depth_noise_f32")
    return out


def depth_noise_batch(items, spec, H=None, W=None):
    """depth_noise for several cameras in one launch.  items = [(clean frames, out frames, word seed, frame ids)]: per item up to 4
    frames, each an [H,W] fp32 tensor or a device pointer (then H and W are needed), which need not be adjacent in memory, and one
    id per frame.  More than 12 items go in chunks of 12."""
    if len(items) > 12:
        for i in range(0, len(items), 12):
            depth_noise_batch(items[i:i + 12], spec, H, W)
        return
    args = _noise_args(spec)
    cl, ou, H, W = _frame_pointers("depth_noise_batch", "clean", [(clean, out, frames) for clean, out, _, frames in items], H, W)
    n = len(cl)
    if n == 0:
        return
    seeds = [int(seed) & 0xFFFFFFFF for _, _, seed, frames in items for _ in frames]
    ids = [int(f) & 0xFFFFFFFF for *_, frames in items for f in frames]
    rc = _lib.lib().nbp_depth_noise_batch_f32(n, (C.c_void_p * n)(*cl), (C.c_void_p * n)(*ou), (C.c_uint * n)(*seeds), (C.c_uint * n)(*ids),
                                              int(H), int(W), *args, _st())
    _lib.check(rc, "nbp_depth_noise_batch_f32")


# ---- the depth-frame filter (csrc/nbp_depth_filter.hip; the definition is utility/depth_filter.py)
def _filter_args(spec):
    from . import depth_filter as df
    spec = df.option_spec(spec)
    if spec is None:
        raise ValueError("depth_filter: a spec is needed (None means off: nothing to launch)")
    return (spec["radius"], spec["range_base"], spec["range_quad"], int(spec["smooth"]), spec["min_support"], spec["fill_support"])


def depth_filter(raw, out, spec):
    """The filter on raw [n,H,W] (or [H,W]) fp32 -> out (same shape, another buffer), frame by frame; spec:
    depth_filter.option_spec's dict.  One launch.  Returns out."""
    if raw.dtype != torch.float32 or out.dtype != torch.float32 or raw.shape != out.shape or raw.dim() not in (2, 3):
        raise ValueError("depth_filter: raw and out are fp32 [n,H,W] (or [H,W]) of one shape")
    n = raw.shape[0] if raw.dim() == 3 else 1
    H, W = raw.shape[-2:]
    rc = _lib.lib().nbp_depth_filter_f32(_lib.ptr(raw), _lib.ptr(out), n, H, W, *_filter_args(spec), _st())
    _lib.check(rc, "nbp_depth_filter_f32")
    return out


def depth_filter_batch(items, spec, H=None, W=None):
    """depth_filter for several cameras in one launch.  items = [(raw frames, out frames)]: per item up to 4 frames, each an [H,W]
    fp32 tensor or a device pointer (then H and W are needed), which need not be adjacent in memory.  More than 12 items go in
    chunks of 12."""
    if len(items) > 12:
        for i in range(0, len(items), 12):
            depth_filter_batch(items[i:i + 12], spec, H, W)
        return
    args = _filter_args(spec)
    ra, ou, H, W = _frame_pointers("depth_filter_batch", "raw", [(raw, out, None) for raw, out in items], H, W)
    n = len(ra)
    if n == 0:
        return
    rc = _lib.lib().nbp_depth_filter_batch_f32(n, (C.c_void_p * n)(*ra), (C.c_void_p * n)(*ou), int(H), int(W), *args, _st())
    _lib.check(rc, "nbp_depth_filter_batch_f32")


def carve_update(proxy_pts, depth, mask, cam12_host, zfar, fov_range, tol, score_threshold, n_inside, n_behind, occ,
                 out_of_field, tan_half_fov=TAN_HALF_FOV):
    """A20 (macarons_utils.py:2849-2949, 3329-3363): in-place update of the per-proxy-point carving state."""
    H, W = depth.shape[-2:]
    cam = (C.c_float * 12)(*[float(x) for x in cam12_host])
    rc = _lib.lib().nbp_carve_update_f32(_lib.ptr(proxy_pts), proxy_pts.shape[0], _lib.ptr(depth), _lib.ptr(mask), cam, H, W,
                                         tan_half_fov, float(zfar), float(fov_range), float(tol), float(score_threshold),
                                         _lib.ptr(n_inside), _lib.ptr(n_behind), _lib.ptr(occ), _lib.ptr(out_of_field),
                                         _st())
    _lib.check(rc, "nbp_carve_update_f32")


def camera_center(cam12_host):
    """World position of the camera of a [12] host camera (R row-major, T): C = -T R^T in fp32 (get_camera_center)."""
    import numpy as np
    c = np.asarray(cam12_host, np.float32)
    R, T = c[:9].reshape(3, 3), c[9:]
    return np.array([-((T[0] * R[j, 0] + T[1] * R[j, 1]) + T[2] * R[j, 2]) for j in range(3)], np.float32)


def view_state_update(pts, x_view_host, n_elev, n_azim, view_states, mask=None, sd=None, distance_to_surface=0.0):
    """compute_view_state (scone_utils.py:799-862) OR-ed into view_states [P, n_elev * n_azim] (fp32 0 / 1) for the selected
    points: mask [P] uint8 (None = all) and sd [P] < distance_to_surface (None = no test); x_view_host [n_view <= 8, 3]."""
    import numpy as np
    xv = np.ascontiguousarray(x_view_host, np.float32).reshape(-1, 3)
    rc = _lib.lib().nbp_view_state_update_f32(_lib.ptr(pts), pts.shape[0], _lib.ptr(mask), _lib.ptr(sd), float(distance_to_surface),
                                              xv.ctypes.data_as(C.POINTER(C.c_float)), len(xv), int(n_elev), int(n_azim),
                                              _lib.ptr(view_states), _st())
    _lib.check(rc, "nbp_view_state_update_f32")


def view_gain(proxy_pts, occ, view_states, cams12_host, x_cams_host, n_elev, n_azim, H, W, fov_range, tan_half_fov=TAN_HALF_FOV):
    """gains [n_cams] int32 (device): occupied proxy points in each candidate's field of view not yet seen from its direction."""
    import numpy as np
    cams = np.ascontiguousarray(cams12_host, np.float32).reshape(-1, 12)
    xs = np.ascontiguousarray(x_cams_host, np.float32).reshape(-1, 3)
    gains = torch.empty(len(cams), dtype=torch.int32, device=proxy_pts.device)
    fp = C.POINTER(C.c_float)
    rc = _lib.lib().nbp_view_gain_i32(_lib.ptr(proxy_pts), proxy_pts.shape[0], _lib.ptr(occ), _lib.ptr(view_states),
                                      cams.ctypes.data_as(fp), xs.ctypes.data_as(fp), len(cams), int(n_elev), int(n_azim), int(H), int(W),
                                      tan_half_fov, float(fov_range), _lib.ptr(gains), _st())
    _lib.check(rc, "nbp_view_gain_i32")
    return gains


def carve_view_update(proxy_pts, depth, mask, cam12_host, zfar, fov_range, tol, score_threshold, n_inside, n_behind, occ,
                      out_of_field, x_cam_host, n_elev, n_azim, distance_to_surface, view_states, fov_mask=None, sd=None,
                      tan_half_fov=TAN_HALF_FOV):
    """carve_update + Scene.update_proxy_view_states (macarons_utils.py:3268-3327) for the frame's camera in ONE launch."""
    H, W = depth.shape[-2:]
    cam = (C.c_float * 12)(*[float(x) for x in cam12_host])
    xc = (C.c_float * 3)(*[float(x) for x in x_cam_host])
    rc = _lib.lib().nbp_carve_view_update_f32(_lib.ptr(proxy_pts), proxy_pts.shape[0], _lib.ptr(depth), _lib.ptr(mask), cam, H, W,
                                              tan_half_fov, float(zfar), float(fov_range), float(tol), float(score_threshold),
                                              _lib.ptr(n_inside), _lib.ptr(n_behind), _lib.ptr(occ), _lib.ptr(out_of_field), xc,
                                              int(n_elev), int(n_azim), float(distance_to_surface), _lib.ptr(view_states),
                                              _lib.ptr(fov_mask), _lib.ptr(sd), _st())
    _lib.check(rc, "nbp_carve_view_update_f32")


def _scene_geom(scene):
    import numpy as np
    box = np.ascontiguousarray(scene.box6(), np.float32)
    grid = np.ascontiguousarray(scene.grid3(), np.int32)
    return box, grid, box.ctypes.data_as(C.POINTER(C.c_float)), grid.ctypes.data_as(C.POINTER(C.c_int))


def scene_fill_cells(scene, pts, n_point_min=0, seed=0, n_dev=None):
    """Scene.fill_cells on the device store of `scene` (simulator/scene.py::Scene); pts [n,3] fp32 device."""
    L = _lib.lib()
    box, grid, bp, gp = _scene_geom(scene)
    n = pts.shape[0]
    ws = _workspace("scene_fill", L.nbp_scene_fill_workspace_bytes(bp, gp, scene.cell_capacity, n, scene.cell_resolution),
                    pts.device)
    rc = L.nbp_scene_fill_cells_f32(_lib.ptr(pts), n, _lib.ptr(n_dev), bp, gp, scene.cell_capacity,
                                    float(scene.cell_resolution), int(n_point_min), int(seed) & 0xFFFFFFFF,
                                    _lib.ptr(scene.cell_pts), _lib.ptr(scene.cell_count), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_scene_fill_cells_f32")


def scene_gather(scene):
    """Scene.return_entire_pt_cloud -> [G,3] device tensor (one sync to size the result)."""
    cap_total = scene.n_cells * scene.cell_capacity
    out = torch.empty(cap_total, 3, dtype=torch.float32, device=scene.cell_pts.device)
    n_out = torch.zeros(1, dtype=torch.int64, device=out.device)
    rc = _lib.lib().nbp_scene_gather_f32(_lib.ptr(scene.cell_pts), _lib.ptr(scene.cell_count), scene.n_cells,
                                         scene.cell_capacity, _lib.ptr(out), cap_total, _lib.ptr(n_out), _st())
    _lib.check(rc, "nbp_scene_gather_f32")
    return out[:int(n_out.item())].clone()


def scene_coverage(gt_scene, rec_scene, epsilon, out=None):
    """-> int32 [2] device: (covered GT points, stored GT points)."""
    L = _lib.lib()
    box, grid, bp, gp = _scene_geom(gt_scene)
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=gt_scene.cell_pts.device)
    ws = _workspace("scene_cov", L.nbp_scene_coverage_workspace_bytes(bp, gp, rec_scene.cell_capacity, float(epsilon)),
                    out.device)
    rc = L.nbp_scene_coverage_f32(_lib.ptr(gt_scene.cell_pts), _lib.ptr(gt_scene.cell_count), gt_scene.cell_capacity,
                                  _lib.ptr(rec_scene.cell_pts), _lib.ptr(rec_scene.cell_count), rec_scene.cell_capacity,
                                  bp, gp, float(epsilon), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_scene_coverage_f32")
    return out


def points_in_fov(pts, cams, H, W, fov_range, want_mask=True, tan_half_fov=TAN_HALF_FOV):
    """Camera.get_points_in_fov for n cameras (host [n,12]) -> (mask uint8 [n,P] or None, any int32 [n])."""
    keep, cam_ptr, n = _cam_arg(cams)
    P = pts.shape[0]
    mask = torch.empty(n, P, dtype=torch.uint8, device=pts.device) if want_mask else None
    any_ = torch.empty(n, dtype=torch.int32, device=pts.device)
    rc = _lib.lib().nbp_points_in_fov_u8(_lib.ptr(pts), P, cam_ptr, n, H, W, tan_half_fov, float(fov_range), _lib.ptr(mask),
                                         _lib.ptr(any_), _st())
    _lib.check(rc, "nbp_points_in_fov_u8")
    return mask, any_


def sample_points(pc, k, seed=0, n_dev=None, n=None):
    """The first k points of a seeded random permutation of pc[:n] -> (out [k,3] device, m int64[1] device)."""
    N = pc.shape[0] if n is None else int(n)
    out = torch.empty(min(int(k), N), 3, dtype=torch.float32, device=pc.device)
    m = torch.zeros(1, dtype=torch.int64, device=pc.device)
    rc = _lib.lib().nbp_sample_points_f32(_lib.ptr(pc), N, _lib.ptr(n_dev), int(k), int(seed) & 0xFFFFFFFF, _lib.ptr(out),
                                          _lib.ptr(m), _st())
    _lib.check(rc, "nbp_sample_points_f32")
    return out, m


def append_points(dst, offset, pts_host):
    """dst[offset:offset+n] = pts (n <= 8 host points, passed in the kernel arguments)."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(pts_host, np.float32).reshape(-1, 3))
    rc = _lib.lib().nbp_append_points_f32(_lib.ptr(dst), int(offset), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], _st())
    _lib.check(rc, "nbp_append_points_f32")


def augment_batch(x, gt, ops):
    """x [B,5,S,S], gt [B,1,S,S] fp32 and ops int32 [B] (op codes of utility/augment.py), all on the device -> (x', gt'): every
    sample's six planes moved by its element of D4 about the camera, one launch (nbp_augment_batch_f32), out of place."""
    for name, t in (("x", x), ("gt", gt), ("ops", ops)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"augment_batch: the HIP path needs a cuda tensor for {name} (no CPU fallback)")
    B, S = x.shape[0], x.shape[-1]
    if (x.dtype != torch.float32 or gt.dtype != torch.float32 or ops.dtype != torch.int32 or tuple(x.shape) != (B, 5, S, S)
            or tuple(gt.shape) != (B, 1, S, S) or tuple(ops.shape) != (B,)):
        raise ValueError("augment_batch: x [B,5,S,S] fp32, gt [B,1,S,S] fp32 and ops [B] int32 expected")
    x_out, gt_out = torch.empty_like(x), torch.empty_like(gt)
    with torch.cuda.device(x.device):
        rc = _lib.lib().nbp_augment_batch_f32(_lib.ptr(x), _lib.ptr(gt), _lib.ptr(ops), B, S, _lib.ptr(x_out), _lib.ptr(gt_out), _st())
    _lib.check(rc, "nbp_augment_batch_f32")
    return x_out, gt_out


_ensemble_ops = {}


def symmetry_ops(ops, device):
    """The op codes of a symmetry ensemble (utility/augment.py::check_ensemble) as a device int32 tensor, one per (device, tuple):
    uploaded at first use, so a step loop -- or a graph capture behind a warm-up -- uploads nothing."""
    from . import augment
    ops = augment.check_ensemble(ops)
    if ops is None:
        raise ValueError("symmetry_ops: an ensemble expected, got None")
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), ops)
    t = _ensemble_ops.get(key)
    if t is None:
        t = _ensemble_ops[key] = torch.tensor(ops, dtype=torch.int32, device=device)
    return t


def _ensemble_args(what, ops, *tensors):
    for name, t in tensors + (("ops", ops),):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: the HIP path needs a cuda tensor for {name} (no CPU fallback)")
    if ops.dtype != torch.int32 or ops.dim() != 1 or not 1 <= ops.shape[0] <= 8:
        raise ValueError(f"{what}: ops is an int32 tensor of 1..8 op codes")
    for name, t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor")
    return int(ops.shape[0])


def symmetry_expand(x, ops, out=None):
    """x [B,5,S,S] fp32 and ops int32 [n] (symmetry_ops), on the device -> x_out [n,B,5,S,S], x_out[k][b] = ops[k] applied to x[b]
    about the camera: one launch (nbp_ensemble_expand_f32), out of place.  out: a caller-owned result tensor (graph capture)."""
    n = _ensemble_args("symmetry_expand", ops, ("x", x), *((("out", out),) if out is not None else ()))
    B, S = (x.shape[0], x.shape[-1]) if x.dim() == 4 else (0, 0)
    if tuple(x.shape) != (B, 5, S, S) or B < 1 or S % 16:
        raise ValueError("symmetry_expand: x [B,5,S,S] fp32 with S % 16 == 0 expected")
    if out is None:
        out = torch.empty(n, B, 5, S, S, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, B, 5, S, S):
        raise ValueError("symmetry_expand: out [n,B,5,S,S] expected")
    with torch.cuda.device(x.device):
        rc = _lib.lib().nbp_ensemble_expand_f32(_lib.ptr(x), B, S, _lib.ptr(ops), n, _lib.ptr(out), _st())
    _lib.check(rc, "nbp_ensemble_expand_f32")
    return out


def symmetry_reduce(raw1, raw2, ops, out=None):
    """raw1 [n,B,8,S/4,S/4] and raw2 [n,B,1,S,S] fp32, the network's outputs on symmetry_expand's batch, and ops int32 [n] ->
    (out1 [B,8,S/4,S/4], out2 [B,1,S,S]): every member moved back by its inverse element and averaged over the members that reach
    the cell (utility/augment.py::ensemble_reference); one launch (nbp_ensemble_reduce_f32).  out = (out1, out2): caller-owned."""
    tensors = (("raw1", raw1), ("raw2", raw2)) + ((("out1", out[0]), ("out2", out[1])) if out is not None else ())
    n = _ensemble_args("symmetry_reduce", ops, *tensors)
    if raw1.dim() != 5 or raw2.dim() != 5:
        raise ValueError("symmetry_reduce: raw1 [n,B,8,S/4,S/4] and raw2 [n,B,1,S,S] expected")
    B, S = raw2.shape[1], raw2.shape[-1]
    if tuple(raw2.shape) != (n, B, 1, S, S) or B < 1 or S % 16 or tuple(raw1.shape) != (n, B, 8, S // 4, S // 4):
        raise ValueError("symmetry_reduce: raw1 [n,B,8,S/4,S/4] and raw2 [n,B,1,S,S] with S % 16 == 0 and n = len(ops) expected")
    if out is None:
        out1 = torch.empty(B, 8, S // 4, S // 4, dtype=torch.float32, device=raw1.device)
        out2 = torch.empty(B, 1, S, S, dtype=torch.float32, device=raw1.device)
    else:
        out1, out2 = out
        if tuple(out1.shape) != (B, 8, S // 4, S // 4) or tuple(out2.shape) != (B, 1, S, S):
            raise ValueError("symmetry_reduce: out = (out1 [B,8,S/4,S/4], out2 [B,1,S,S]) expected")
    with torch.cuda.device(raw1.device):
        rc = _lib.lib().nbp_ensemble_reduce_f32(_lib.ptr(raw1), _lib.ptr(raw2), B, S, _lib.ptr(ops), n, _lib.ptr(out1), _lib.ptr(out2),
                                                _st())
    _lib.check(rc, "nbp_ensemble_reduce_f32")
    return out1, out2


def replay_stream_bound(S):
    """Largest compact stream of a record of side S (nbp_replay_stream_bound; utility/replay_codec.py::stream_bound)."""
    n = int(_lib.lib().nbp_replay_stream_bound(int(S)))
    if n == 0:
        raise ValueError(f"replay_stream_bound: S = {S} is not a multiple of 16 in 16..512")
    return n


def replay_encode(rec, arena=None):
    """rec [n,6,S,S] fp32 on the device (five input maps + the obstacle label per record) -> arena [n, stride] uint8 on the device:
    row r starts with record r's compact stream (utility/replay_codec.py's bytes; its header holds total_bytes), the rest of the
    row is left as it was.  Two launches (nbp_replay_encode_f32), no host synchronisation.  arena: a caller-owned [n, stride]
    uint8 tensor with stride >= replay_stream_bound(S), a multiple of 16."""
    if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
        raise RuntimeError("replay_encode: the HIP path needs a cuda tensor for rec (no CPU fallback)")
    if rec.dtype != torch.float32 or rec.dim() != 4 or rec.shape[1] != 6 or rec.shape[2] != rec.shape[3] or rec.shape[0] < 1:
        raise ValueError("replay_encode: rec [n,6,S,S] fp32 expected")
    n, S = rec.shape[0], rec.shape[-1]
    if arena is None:
        arena = torch.empty(n, replay_stream_bound(S), dtype=torch.uint8, device=rec.device)
    elif (not isinstance(arena, torch.Tensor) or not arena.is_cuda or arena.dtype != torch.uint8 or arena.dim() != 2
          or arena.shape[0] != n):
        raise ValueError("replay_encode: arena [n, stride] uint8 on the device expected")
    with torch.cuda.device(rec.device):
        rc = _lib.lib().nbp_replay_encode_f32(_lib.ptr(rec), n, S, _lib.ptr(arena), int(arena.shape[1]), _st())
    _lib.check(rc, "nbp_replay_encode_f32")
    return arena


def replay_decode(streams, offsets, S, out=None):
    """streams: a uint8 device buffer that holds n compact streams at the byte offsets `offsets` (a host sequence of ints, each a
    multiple of 16), headers already validated by the host (replay_codec.parse_header) -> (x [n,5,S,S], gt [n,1,S,S]) fp32, every
    pixel written: one launch (nbp_replay_decode_f32; per 64 records).  out = (x, gt): caller-owned results."""
    if not isinstance(streams, torch.Tensor) or not streams.is_cuda:
        raise RuntimeError("replay_decode: the HIP path needs a cuda tensor for streams (no CPU fallback)")
    if streams.dtype != torch.uint8 or streams.dim() != 1:
        raise ValueError("replay_decode: streams is a flat uint8 tensor")
    offs = [int(o) for o in offsets]
    n = len(offs)
    if n < 1 or min(offs) < 0 or max(offs) + 64 > streams.numel():
        raise ValueError("replay_decode: 1 or more offsets inside the buffer expected")
    if out is None:
        x = torch.empty(n, 5, S, S, dtype=torch.float32, device=streams.device)
        gt = torch.empty(n, 1, S, S, dtype=torch.float32, device=streams.device)
    else:
        x, gt = out
        if (x.dtype != torch.float32 or gt.dtype != torch.float32 or tuple(x.shape) != (n, 5, S, S)
                or tuple(gt.shape) != (n, 1, S, S) or x.device != streams.device or gt.device != streams.device):
            raise ValueError("replay_decode: out = (x [n,5,S,S], gt [n,1,S,S]) fp32 on the streams' device expected")
    arr = (C.c_longlong * n)(*offs)
    with torch.cuda.device(streams.device):
        rc = _lib.lib().nbp_replay_decode_f32(_lib.ptr(streams), arr, n, int(S), _lib.ptr(x), _lib.ptr(gt), _st())
    _lib.check(rc, "nbp_replay_decode_f32")
    return x, gt


def validation_metrics(out1, out2, gt, coords, gains, bidx, thresholds=(0.13,)):
    """One validation batch on the device -> (obst int64 [B,T,4], rank int64 [B,6], val float64 [B,4]) on the device: the per-sample
    quantities of utility/metrics.py::validation_metrics_reference (the obstacle mask `out2 >= threshold` against `gt > 0.5`; the
    ranking of the supervised cells of out1 against their gains).  out1 [B,8,S/4,S/4], out2 / gt [B,1,S,S] fp32, coords [K,3] int64,
    gains [K] fp32, bidx [K] int64 (any order), thresholds: 1 to 8 numbers.  One memset and two launches on the current stream
    (nbp_val_metrics_f32), no host synchronisation.  K = 0 is legal."""
    from . import metrics
    ts = metrics.check_thresholds(thresholds)
    named = (("out1", out1), ("out2", out2), ("gt", gt), ("coords", coords), ("gains", gains), ("bidx", bidx))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"validation_metrics: the HIP path needs a cuda tensor for {name} (no CPU fallback)")
    if out2.dim() != 4 or out1.dim() != 4:
        raise ValueError("validation_metrics: out1 [B,8,S/4,S/4] and out2 [B,1,S,S] expected")
    B, S = out2.shape[0], out2.shape[-1]
    K = coords.shape[0] if coords.dim() == 2 else -1
    if (B < 1 or S < 4 or S % 4 or tuple(out2.shape) != (B, 1, S, S) or tuple(gt.shape) != (B, 1, S, S)
            or tuple(out1.shape) != (B, 8, S // 4, S // 4) or tuple(coords.shape) != (K, 3) or tuple(gains.shape) != (K,)
            or tuple(bidx.shape) != (K,)):
        raise ValueError("validation_metrics: out1 [B,8,S/4,S/4], out2 / gt [B,1,S,S], coords [K,3], gains [K] and bidx [K] expected")
    if (out1.dtype != torch.float32 or out2.dtype != torch.float32 or gt.dtype != torch.float32 or gains.dtype != torch.float32
            or coords.dtype != torch.int64 or bidx.dtype != torch.int64):
        raise ValueError("validation_metrics: fp32 out1 / out2 / gt / gains and int64 coords / bidx expected")
    if any(t.device != out2.device for _, t in named):
        raise ValueError("validation_metrics: all tensors on one device expected")
    if not all(t.is_contiguous() for _, t in named):
        raise ValueError("validation_metrics: contiguous tensors expected")
    dev = out2.device
    obst = torch.empty(B, len(ts), 4, dtype=torch.int64, device=dev)
    rank = torch.empty(B, 6, dtype=torch.int64, device=dev)
    val = torch.empty(B, 4, dtype=torch.float64, device=dev)
    th = (C.c_float * len(ts))(*ts)
    with torch.cuda.device(dev):
        rc = _lib.lib().nbp_val_metrics_f32(_lib.ptr(out1), _lib.ptr(out2), _lib.ptr(gt), _lib.ptr(coords), _lib.ptr(gains),
                                            _lib.ptr(bidx), B, S, K, len(ts), th, _lib.ptr(obst), _lib.ptr(rank), _lib.ptr(val), _st())
    _lib.check(rc, "nbp_val_metrics_f32")
    return obst, rank, val


def _objective_args(name, out1, coords_bcxy, gains, out2, gt, weights):
    """Checks the tensors the objective's forward and backward share -> (B, S, C, H, W, K)."""
    named = [("out1", out1), ("coords_bcxy", coords_bcxy), ("gains", gains), ("out2", out2), ("gt", gt)]
    if weights is not None:
        named.append(("weights", weights))
    for n, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: the HIP path needs a cuda tensor for {n} (no CPU fallback)")
    if out1.dim() != 4 or out2.dim() not in (3, 4) or out2.shape[-1] != out2.shape[-2] or (out2.dim() == 4 and out2.shape[1] != 1):
        raise ValueError(f"{name}: out1 [B,C,H,W] and out2 [B,S,S] (or [B,1,S,S]) expected")
    B, C, H, W = out1.shape
    S = out2.shape[-1]
    K = coords_bcxy.shape[0] if coords_bcxy.dim() == 2 else -1
    if (B < 1 or S < 1 or out2.shape[0] != B or gt.shape != out2.shape or tuple(coords_bcxy.shape) != (K, 4)
            or tuple(gains.shape) != (K,) or (weights is not None and tuple(weights.shape) != (B,))):
        raise ValueError(f"{name}: out1 [B,C,H,W], out2 / gt [B,S,S], coords_bcxy [K,4], gains [K] and weights [B] expected")
    if (coords_bcxy.dtype != torch.int64 or any(t.dtype != torch.float32 for n, t in named if n != "coords_bcxy")):
        raise ValueError(f"{name}: fp32 out1 / out2 / gt / gains / weights and int64 coords_bcxy expected")
    if any(t.device != out2.device for _, t in named):
        raise ValueError(f"{name}: all tensors on one device expected")
    if not all(t.is_contiguous() for _, t in named):
        raise ValueError(f"{name}: contiguous tensors expected")
    return B, S, C, H, W, K


def objective_forward(out1, coords_bcxy, gains, out2, gt, weights=None):
    """The training objective's per-sample terms on the device (csrc/nbp_objective.hip; the definition of record is
    utility/priority.py::objective_reference) -> (per_sample float64 [B,3] = (v_b, n_b, o_b), totals float64 [2] =
    (sum w_b v_b, sum w_b o_b)).  out1 [B,C,H,W], out2 / gt [B,S,S] or [B,1,S,S] fp32, coords_bcxy [K,4] int64 (rows in any order),
    gains [K] fp32, weights None or [B] fp32.  Two launches on the current stream, no host synchronisation; K = 0 is legal."""
    B, S, C, H, W, K = _objective_args("objective_forward", out1, coords_bcxy, gains, out2, gt, weights)
    dev = out2.device
    L = _lib.lib()
    per_sample = torch.empty(B, 3, dtype=torch.float64, device=dev)
    totals = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace("objective", L.nbp_objective_workspace_bytes(B, S), dev)
        rc = L.nbp_objective_forward_f32(_lib.ptr(out1), _lib.ptr(coords_bcxy), _lib.ptr(gains), K, C, H, W, _lib.ptr(out2), _lib.ptr(gt),
                                         B, S, _lib.ptr(weights), _lib.ptr(per_sample), _lib.ptr(totals), _lib.ptr(ws), ws.numel(),
                                         _st())
    _lib.check(rc, "nbp_objective_forward_f32")
    return per_sample, totals


def objective_backward(out1, coords_bcxy, gains, out2, gt, weights, coef):
    """The gradients of coef[0] * mse + coef[1] * bce (mse = totals[0] / K, bce = totals[1] / (B S^2)) -> (d_out1, d_out2), shaped as
    out1 and out2.  coef: fp32 [2] ON THE DEVICE, read there: one asynchronous fill and one launch, no host synchronisation."""
    B, S, C, H, W, K = _objective_args("objective_backward", out1, coords_bcxy, gains, out2, gt, weights)
    dev = out2.device
    if (not isinstance(coef, torch.Tensor) or coef.device != dev or coef.dtype != torch.float32 or tuple(coef.shape) != (2,)
            or not coef.is_contiguous()):
        raise ValueError("objective_backward: coef fp32 [2] on the tensors' device expected")
    L = _lib.lib()
    d_out1 = torch.empty_like(out1)
    d_out2 = torch.empty_like(out2)
    with torch.cuda.device(dev):
        ws = _workspace("objective", L.nbp_objective_workspace_bytes(B, S), dev)
        rc = L.nbp_objective_backward_f32(_lib.ptr(out1), _lib.ptr(coords_bcxy), _lib.ptr(gains), K, C, H, W, _lib.ptr(out2),
                                          _lib.ptr(gt), B, S, _lib.ptr(weights), _lib.ptr(coef), _lib.ptr(d_out1), _lib.ptr(d_out2),
                                          _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_objective_backward_f32")
    return d_out1, d_out2


# ---- reconstruction-quality metrics (csrc/nbp_recon.hip; the definition of record is utility/recon_metrics.py)
def _nn_points(name, t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a cuda tensor for {what} (no CPU fallback)")
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous fp32 [n,3] tensor")


def _nn_count(name, n_dev, device):
    if n_dev is not None and (not isinstance(n_dev, torch.Tensor) or n_dev.device != device or n_dev.dtype != torch.int64
                              or n_dev.numel() != 1):
        raise ValueError(f"{name}: a device counter is one int64 element on the points' device")


def _nn_box(box):
    lo, hi = box
    return (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi])


def _nn_out(name, out, n, device):
    if out is None:
        return torch.empty(n, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or out.device != device or out.dim() != 1 or out.shape[0] < n or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous fp32 tensor of at least {n} elements on the points' device")
    return out


def nn_dist2(query, target, box, cap, cell=1.0, n_query_dev=None, n_target_dev=None, out=None):
    """Truncated exact nearest-neighbour squared distances -> fp32 [Q] on the device: out[i] = min(cap^2, min over the targets inside
    box = (lo, hi) of |t - q_i|^2), bit for bit recon_metrics.nn_dist2_reference.  query [Q,3], target [T,3] fp32; n_query_dev /
    n_target_dev: int64 device counters (rows beyond them are never read, entries of out beyond n_query_dev never written).  The
    targets are sorted into a grid of `cell`-wide cells per call (NNPlan sorts a static set once).  No host synchronisation."""
    _nn_points("nn_dist2", query, "query")
    _nn_points("nn_dist2", target, "target")
    if target.device != query.device:
        raise ValueError("nn_dist2: query and target on one device expected")
    _nn_count("nn_dist2", n_query_dev, query.device)
    _nn_count("nn_dist2", n_target_dev, query.device)
    L = _lib.lib()
    lo, hi = _nn_box(box)
    Q, T = query.shape[0], target.shape[0]
    out = _nn_out("nn_dist2", out, Q, query.device)
    with torch.cuda.device(query.device):
        nbytes = L.nbp_nn_dist2_workspace_bytes(lo, hi, float(cell), T)
        ws = _workspace("nn_dist2", nbytes, query.device)
        # (a zero size: the call names the reason -- its argument and shape checks come before the workspace's)
        rc = L.nbp_nn_dist2_f32(_lib.ptr(query), Q, _lib.ptr(n_query_dev), _lib.ptr(target), T, _lib.ptr(n_target_dev), lo, hi,
                                float(cap), float(cell), _lib.ptr(out), _lib.ptr(ws), ws.numel() if nbytes else 0, _st())
    _lib.check(rc, "nbp_nn_dist2_f32")
    return out


class NNPlan:
    """A static target set sorted once into the nearest-neighbour grid (nbp_nn_plan_build_f32); `dist2` then costs one launch."""

    def __init__(self, target, box, cell=1.0, n_target_dev=None):
        _nn_points("NNPlan", target, "target")
        _nn_count("NNPlan", n_target_dev, target.device)
        L = _lib.lib()
        self.target, self.cell, self.T = target, float(cell), target.shape[0]
        self.lo, self.hi = _nn_box(box)
        with torch.cuda.device(target.device):
            nplan = L.nbp_nn_plan_bytes(self.lo, self.hi, self.cell, self.T)
            nws = L.nbp_nn_plan_workspace_bytes(self.lo, self.hi, self.cell, self.T)
            # (a zero size: the build call names the reason)
            self.plan = torch.empty(max(nplan, 256), dtype=torch.uint8, device=target.device)
            ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=target.device)
            rc = L.nbp_nn_plan_build_f32(_lib.ptr(target), self.T, _lib.ptr(n_target_dev), self.lo, self.hi, self.cell,
                                         _lib.ptr(self.plan), nplan, _lib.ptr(ws), nws, _st())
        _lib.check(rc, "nbp_nn_plan_build_f32")

    def dist2(self, query, cap, n_query_dev=None, out=None):
        """nn_dist2(query, the plan's targets, ...) without the sort."""
        _nn_points("NNPlan.dist2", query, "query")
        if query.device != self.plan.device:
            raise ValueError("NNPlan.dist2: query on the plan's device expected")
        _nn_count("NNPlan.dist2", n_query_dev, query.device)
        Q = query.shape[0]
        out = _nn_out("NNPlan.dist2", out, Q, query.device)
        with torch.cuda.device(query.device):
            rc = _lib.lib().nbp_nn_dist2_planned_f32(_lib.ptr(self.plan), self.lo, self.hi, self.cell, float(cap), _lib.ptr(query), Q,
                                                     _lib.ptr(n_query_dev), _lib.ptr(out), _st())
        _lib.check(rc, "nbp_nn_dist2_planned_f32")
        return out


def recon_stats(d2, thresholds, n_dev=None):
    """Summary of squared distances d2 fp32 [n] (n_dev: int64 device counter; the tail beyond it is ignored) -> (sums float64 [2] =
    (sum sqrt(d2), sum d2), counts int64 [T] = #{sqrt(d2) < threshold}) on the device; 1 to 8 thresholds.  Two launches, no
    floating-point atomics (two calls give the same bits), no host synchronisation."""
    from . import recon_metrics
    if not isinstance(d2, torch.Tensor) or not d2.is_cuda:
        raise RuntimeError("recon_stats: the HIP path needs a cuda tensor for d2 (no CPU fallback)")
    if d2.dim() != 1 or d2.dtype != torch.float32 or not d2.is_contiguous():
        raise ValueError("recon_stats: d2 must be a contiguous fp32 [n] tensor")
    ts = [float(t) for t in thresholds]
    if not 1 <= len(ts) <= recon_metrics.MAX_THRESHOLDS:
        raise ValueError(f"recon_stats: 1 to {recon_metrics.MAX_THRESHOLDS} thresholds expected, got {len(ts)}")
    _nn_count("recon_stats", n_dev, d2.device)
    L = _lib.lib()
    sums = torch.empty(2, dtype=torch.float64, device=d2.device)
    counts = torch.empty(len(ts), dtype=torch.int64, device=d2.device)
    th = (C.c_float * len(ts))(*ts)
    with torch.cuda.device(d2.device):
        ws = _workspace_for("recon_stats", 0, L.nbp_recon_stats_workspace_bytes, d2.device)
        rc = L.nbp_recon_stats_f64(_lib.ptr(d2), d2.shape[0], _lib.ptr(n_dev), len(ts), th, _lib.ptr(sums), _lib.ptr(counts),
                                   _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_recon_stats_f64")
    return sums, counts


class ReconMetrics:
    """Accuracy, completeness, Chamfer distance and precision / recall / F-score of a cloud against a GT surface, on the device.
    The GT [G,3] is sorted once (its plan serves cloud -> GT); GT -> cloud sorts the cloud per evaluation.  bbox = (lo, hi) of the
    GT on the host; both directions work inside it grown by `cap` (recon_metrics.grown_box)."""

    def __init__(self, gt, bbox, thresholds=(1.0,), cap=5.0, cell=1.0):
        from . import recon_metrics
        self.thresholds, self.cap, self.cell = recon_metrics.check_options(thresholds, cap, cell)
        _nn_points("ReconMetrics", gt, "gt")
        if gt.shape[0] < 1:
            raise ValueError("ReconMetrics: an empty GT surface")
        self.gt, self.G = gt, gt.shape[0]
        lo, hi = recon_metrics.grown_box(bbox[0], bbox[1], self.cap)
        self.box = (lo.tolist(), hi.tolist())
        self.plan = NNPlan(gt, self.box, self.cell)
        self.result = None

    def evaluate(self, cloud, n_dev=None):
        """Enqueues both directions and their summaries on the current stream -> dict of device tensors (acc_sums / comp_sums float64
        [2], acc_counts / comp_counts int64 [T], n_points int64 [1]); no host synchronisation.  Kept for summary() / raw()."""
        _nn_points("ReconMetrics.evaluate", cloud, "cloud")
        dev, N = cloud.device, cloud.shape[0]
        # the distances are scratch of the stream (consumed by the summaries enqueued right behind them)
        d2c = _workspace("recon_d2_cloud", 4 * max(N, 1), dev)[:4 * N].view(torch.float32)
        d2g = _workspace("recon_d2_gt", 4 * self.G, dev)[:4 * self.G].view(torch.float32)
        self.plan.dist2(cloud, self.cap, n_query_dev=n_dev, out=d2c)
        acc_sums, acc_counts = recon_stats(d2c, self.thresholds, n_dev)
        nn_dist2(self.gt, cloud, self.box, self.cap, self.cell, n_target_dev=n_dev, out=d2g)
        comp_sums, comp_counts = recon_stats(d2g, self.thresholds)
        if n_dev is None:
            n_points = torch.full((1,), N, dtype=torch.int64, device=dev)
        else:
            n_points = n_dev.reshape(1).clamp(0, N)          # (a copy: the counter may move on)
        self.result = {"acc_sums": acc_sums, "acc_counts": acc_counts, "comp_sums": comp_sums, "comp_counts": comp_counts,
                       "n_points": n_points}
        return self.result

    def raw(self):
        """The last evaluation's raw numbers on the host (ONE device -> host copy): recon_metrics.pack_raw's float64 vector."""
        from . import recon_metrics
        if self.result is None:
            raise RuntimeError("ReconMetrics: evaluate() first")
        r = self.result
        T = len(self.thresholds)
        flat = torch.cat([r["acc_sums"], r["comp_sums"], r["n_points"].double(), r["acc_counts"].double(),
                          r["comp_counts"].double()]).cpu().numpy()
        return recon_metrics.pack_raw(flat[0:2], flat[5:5 + T], flat[4], flat[2:4], flat[5 + T:5 + 2 * T], self.G)

    def summary(self):
        """The last evaluation as the dict of recon_metrics.summarise (ratios formed on the host from the raw sums and counts)."""
        from . import recon_metrics
        return recon_metrics.summarise_raw(self.raw(), self.thresholds, self.cap)


# ---- cloud-to-mesh accuracy (csrc/nbp_surface.hip; the definition of record is utility/surface_metrics.py)
class MeshPlan:
    """The triangles of a mesh inside `box` = (lo, hi) registered once in the grid of `cell`-wide cells (nbp_mesh_plan_count_f32 /
    nbp_mesh_plan_fill_i32); `dist2` then costs one launch.  verts fp32 [V,3], faces int32 [F,3] on the device.  Construction reads
    the number of (triangle, cell) pairs back: the ONE host synchronisation of this path, at setup.  `entries` = that number,
    `faces_used` = the triangles that take part (surface_metrics.participating)."""

    def __init__(self, verts, faces, box, cell=1.0):
        _nn_points("MeshPlan", verts, "verts")
        if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
            raise RuntimeError("MeshPlan: the HIP path needs a cuda tensor for faces (no CPU fallback)")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or not faces.is_contiguous():
            raise ValueError("MeshPlan: faces must be a contiguous int32 [n,3] tensor")
        if faces.device != verts.device:
            raise ValueError("MeshPlan: verts and faces on one device expected")
        L = _lib.lib()
        dev = verts.device
        self.verts, self.faces, self.cell, self.V, self.F = verts, faces, float(cell), verts.shape[0], faces.shape[0]
        self.lo, self.hi = _nn_box(box)
        with torch.cuda.device(dev):
            nplan = L.nbp_mesh_plan_bytes(self.lo, self.hi, self.cell, self.F)
            nws = L.nbp_mesh_plan_workspace_bytes(self.lo, self.hi, self.cell)
            # (a zero size: the count call names the reason)
            self.plan = torch.empty(max(nplan, 256), dtype=torch.uint8, device=dev)
            ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
            totals = torch.empty(2, dtype=torch.int64, device=dev)
            args = (_lib.ptr(verts), self.V, _lib.ptr(faces), self.F, self.lo, self.hi, self.cell, _lib.ptr(self.plan))
            rc = L.nbp_mesh_plan_count_f32(*args, nplan, _lib.ptr(totals), _lib.ptr(ws), nws, _st())
            _lib.check(rc, "nbp_mesh_plan_count_f32")
            self.entries, self.faces_used = (int(v) for v in totals.tolist())          # the host synchronisation
            fits = self.entries <= 0x7fffffff     # (beyond: no list is allocated, and the fill call names the reason)
            self.entry_list = torch.empty(max(self.entries, 1) if fits else 1, dtype=torch.int32, device=dev)
            rc = L.nbp_mesh_plan_fill_i32(*args, _lib.ptr(self.entry_list), self.entries, _lib.ptr(ws), nws, _st())
        _lib.check(rc, "nbp_mesh_plan_fill_i32")

    def dist2(self, query, cap, n_query_dev=None, out=None):
        """Truncated exact squared distances to the mesh -> fp32 [Q] on the device: out[i] = min(cap^2, min over the plan's triangles
        of point_triangle_d2(q_i, ...)), bit for bit surface_metrics.mesh_dist2_reference.  n_query_dev: int64 device counter (rows
        beyond it are never read, entries of out beyond it never written).  One launch, no host synchronisation."""
        _nn_points("MeshPlan.dist2", query, "query")
        if query.device != self.plan.device:
            raise ValueError("MeshPlan.dist2: query on the plan's device expected")
        _nn_count("MeshPlan.dist2", n_query_dev, query.device)
        Q = query.shape[0]
        out = _nn_out("MeshPlan.dist2", out, Q, query.device)
        with torch.cuda.device(query.device):
            rc = _lib.lib().nbp_mesh_dist2_planned_f32(_lib.ptr(self.plan), _lib.ptr(self.entry_list), self.lo, self.hi, self.cell,
                                                       float(cap), _lib.ptr(query), Q, _lib.ptr(n_query_dev), _lib.ptr(out), _st())
        _lib.check(rc, "nbp_mesh_dist2_planned_f32")
        return out


def mesh_dist2(query, verts, faces, box, cap, cell=1.0, n_query_dev=None, out=None):
    """MeshPlan(verts, faces, box, cell).dist2(query, cap, ...): the plan built for one call (its build synchronises with the host)."""
    return MeshPlan(verts, faces, box, cell).dist2(query, cap, n_query_dev=n_query_dev, out=out)


class SurfaceMetrics:
    """Accuracy of a cloud against the surface of a mesh (not a sample of it), on the device: the mean and RMS truncated distance to
    the nearest triangle and the share of points within each threshold (utility/surface_metrics.py).  mesh: an object with verts
    fp32 [V,3] and faces int32 [F,3] on the device and verts_host (simulator/scene.py::DeviceMesh); the triangles are registered
    once, inside the vertex bounds grown by `cap` (surface_metrics.mesh_box)."""

    def __init__(self, mesh, thresholds=None, cap=5.0, cell=1.0):
        from . import surface_metrics
        thresholds = surface_metrics.DEFAULT_THRESHOLDS if thresholds is None else thresholds
        self.thresholds, self.cap, self.cell = surface_metrics.check_options(thresholds, cap, cell)
        lo, hi = surface_metrics.mesh_box(mesh.verts_host, self.cap)
        self.box = (lo.tolist(), hi.tolist())
        self.plan = MeshPlan(mesh.verts, mesh.faces, self.box, self.cell)
        self.result = None

    def evaluate(self, cloud, n_dev=None):
        """Enqueues the distances and their summary on the current stream -> dict of device tensors (sums float64 [2], counts int64
        [T], n_points int64 [1]); no host synchronisation.  Kept for summary() / raw()."""
        _nn_points("SurfaceMetrics.evaluate", cloud, "cloud")
        dev, N = cloud.device, cloud.shape[0]
        # the distances are scratch of the stream (consumed by the summary enqueued right behind them)
        d2 = _workspace("surface_d2_cloud", 4 * max(N, 1), dev)[:4 * N].view(torch.float32)
        self.plan.dist2(cloud, self.cap, n_query_dev=n_dev, out=d2)
        sums, counts = recon_stats(d2, self.thresholds, n_dev)
        if n_dev is None:
            n_points = torch.full((1,), N, dtype=torch.int64, device=dev)
        else:
            n_points = n_dev.reshape(1).clamp(0, N)          # (a copy: the counter may move on)
        self.result = {"sums": sums, "counts": counts, "n_points": n_points}
        return self.result

    def raw(self):
        """The last evaluation's raw numbers on the host (ONE device -> host copy): surface_metrics.pack_raw's float64 vector."""
        from . import surface_metrics
        if self.result is None:
            raise RuntimeError("SurfaceMetrics: evaluate() first")
        r = self.result
        flat = torch.cat([r["sums"], r["n_points"].double(), r["counts"].double()]).cpu().numpy()
        return surface_metrics.pack_raw(flat[0:2], flat[3:], flat[2])

    def summary(self):
        """The last evaluation as the dict of surface_metrics.summarise_raw (ratios formed on the host from the raw sums and counts)."""
        from . import surface_metrics
        return surface_metrics.summarise_raw(self.raw(), self.thresholds, self.cap)

    def mesh_block(self):
        """The record's "mesh" entry: the triangles of the mesh, those that take part, and the grid's (triangle, cell) pairs."""
        return {"faces": self.plan.F, "faces_used": self.plan.faces_used, "entries": self.plan.entries}


_CurveItem = collections.namedtuple("_CurveItem", "curve cloud n_dev row new_bound")      # what ReconCurve.item hands out


class ReconCurve:
    """The reconstruction metrics after every step of a rollout, updated incrementally on the device (recon_metrics.CurveReference is
    the definition; csrc/nbp_recon.hip the kernels).  Owns the running per-GT-point minimum `d2_gt` fp32 [G] (the GT's order), the
    watermark `seen` (int64: the cloud rows already taken in), the running accuracy totals and `rows` float64 [n_rows, 6 + 2 T]
    (recon_metrics.pack_raw's layout).  n_rows defaults to a row per step of a rollout and a spare (lockstep.N_POSES + 1).
    bbox = (lo, hi) of the GT on the host: it has to hold every GT point (checked once, here).  plan: the NNPlan of a ReconMetrics
    over the same GT, box and cell, shared instead of sorting the GT again."""

    def __init__(self, gt, bbox, thresholds=(1.0,), cap=5.0, cell=1.0, n_rows=102, plan=None):
        from . import recon_metrics
        self.thresholds, self.cap, self.cell = recon_metrics.check_options(thresholds, cap, cell)
        _nn_points("ReconCurve", gt, "gt")
        if gt.shape[0] < 1:
            raise ValueError("ReconCurve: an empty GT surface")
        if int(n_rows) < 1:
            raise ValueError("ReconCurve: n_rows >= 1 expected")
        self.gt, self.G, self.n_rows = gt, gt.shape[0], int(n_rows)
        dev = gt.device
        blo, bhi = torch.tensor(bbox[0], dtype=torch.float32, device=dev), torch.tensor(bbox[1], dtype=torch.float32, device=dev)
        if tuple(blo.shape) != (3,) or tuple(bhi.shape) != (3,) or not bool(((gt >= blo) & (gt <= bhi)).all()):
            raise ValueError("ReconCurve: bbox = (lo [3], hi [3]) holding every GT point expected")
        lo, hi = recon_metrics.grown_box(bbox[0], bbox[1], self.cap)
        self.box = (lo.tolist(), hi.tolist())
        if plan is None:
            plan = NNPlan(gt, self.box, self.cell)
        elif (not isinstance(plan, NNPlan) or plan.plan.device != dev or plan.T != self.G or plan.cell != self.cell
              or plan.target.data_ptr() != gt.data_ptr() or [list(plan.lo), list(plan.hi)] != [list(v) for v in _nn_box(self.box)]):
            raise ValueError("ReconCurve: plan must be the NNPlan of the same GT tensor, grown box and cell")
        self.plan = plan
        L = _lib.lib()
        T = len(self.thresholds)
        self.width = recon_metrics.RAW_HEAD + 2 * T
        self.d2_gt = torch.empty(self.G, dtype=torch.float32, device=dev)
        self.seen = torch.zeros(1, dtype=torch.int64, device=dev)
        self.totals = torch.zeros(L.nbp_recon_curve_totals_bytes() // 8, dtype=torch.int64, device=dev)
        self.rows = torch.zeros(self.n_rows, self.width, dtype=torch.float64, device=dev)
        self._d2_new = None                # the new points' own distances: scratch, one entry per cloud row (made by the first item)
        self.reset()

    def reset(self):
        """An empty cloud again: every GT point at the cap, no point seen, zero totals and rows.  Enqueue-only."""
        import numpy as np
        self.d2_gt.fill_(float(np.float32(self.cap) * np.float32(self.cap)))
        self.seen.zero_()
        self.totals.zero_()
        self.rows.zero_()

    def item(self, cloud, n_dev, row, new_bound):
        """The arguments of recon_curve_update_batch for one update: the cloud rows [seen, min(n_dev, capacity)) are taken in and the
        metrics of the cloud so far go into rows[row].  new_bound: host bound of the number of new rows (it only sizes the grid)."""
        _nn_points("ReconCurve.item", cloud, "cloud")
        if cloud.device != self.gt.device:
            raise ValueError("ReconCurve.item: cloud on the GT's device expected")
        if n_dev is None:
            raise ValueError("ReconCurve.item: the cloud's device counter is needed (both ends of the new range are read on the device)")
        _nn_count("ReconCurve.item", n_dev, cloud.device)
        if cloud.shape[0] < 1:
            raise ValueError("ReconCurve.item: a cloud buffer of at least one row expected")
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < self.n_rows:
            raise ValueError(f"ReconCurve.item: row {row!r} outside [0, {self.n_rows})")
        if int(new_bound) < 0:
            raise ValueError("ReconCurve.item: new_bound >= 0 expected")
        if self._d2_new is None or self._d2_new.shape[0] < cloud.shape[0]:
            self._d2_new = torch.empty(cloud.shape[0], dtype=torch.float32, device=cloud.device)
        return _CurveItem(self, cloud, n_dev, row, int(new_bound))

    def update(self, cloud, n_dev, row, new_bound):
        """One update (the batch of one) -> rows[row] on the device."""
        recon_curve_update_batch([self.item(cloud, n_dev, row, new_bound)])
        return self.rows[row]

    def raw(self, n):
        """The first n rows on the host, numpy float64 [n, 6 + 2 T], in ONE device -> host copy."""
        if not 0 <= int(n) <= self.n_rows:
            raise ValueError(f"ReconCurve.raw: n outside [0, {self.n_rows}]")
        return self.rows[:int(n)].cpu().numpy()

    def curve(self, n):
        """The first n rows as recon_metrics.summarise_curve's dict of lists (ratios formed on the host)."""
        from . import recon_metrics
        return recon_metrics.summarise_curve(self.raw(n), self.thresholds, self.cap)


def recon_curve_update_batch(items):
    """ReconCurve.update for several curves (items = [ReconCurve.item(...)]) in three launches whatever their number up to 16; more
    go in chunks of 16.  Each item's results are bit for bit those of a call of its own.  No host synchronisation."""
    import numpy as np
    if not items:
        return
    for it in items:
        if not isinstance(it, _CurveItem):
            raise ValueError("recon_curve_update_batch: items made by ReconCurve.item expected")
    dev = items[0][1].device
    if any(it[1].device != dev for it in items):
        raise ValueError("recon_curve_update_batch: the items of one call on one device expected")
    if len({id(it[0]) for it in items}) != len(items):
        raise ValueError("recon_curve_update_batch: a curve appears twice (its updates are ordered: one call each)")
    if len(items) > 16:
        for i in range(0, len(items), 16):
            recon_curve_update_batch(items[i:i + 16])
        return
    n = len(items)
    VP, LL, I = C.c_void_p, C.c_longlong, C.c_int
    plans, cloud, count, seen, d2g, d2n, tot, row = [(VP * n)() for _ in range(8)]
    G, T, capacity, bound = (I * n)(), (I * n)(), (LL * n)(), (LL * n)()
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    cell, cap, th = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 8), np.float32)
    for i, (cv, pc, n_dev, r, nb) in enumerate(items):
        plans[i], cloud[i], count[i], seen[i] = cv.plan.plan.data_ptr(), pc.data_ptr(), n_dev.data_ptr(), cv.seen.data_ptr()
        d2g[i], d2n[i], tot[i], row[i] = cv.d2_gt.data_ptr(), cv._d2_new.data_ptr(), cv.totals.data_ptr(), cv.rows[r].data_ptr()
        G[i], T[i], capacity[i], bound[i] = cv.G, len(cv.thresholds), pc.shape[0], nb
        lo[i], hi[i], cell[i], cap[i] = list(cv.plan.lo), list(cv.plan.hi), cv.cell, cv.cap
        th[i, :len(cv.thresholds)] = cv.thresholds
    L = _lib.lib()
    with torch.cuda.device(dev):
        ws = _workspace_for("recon_curve", 16, lambda: L.nbp_recon_curve_workspace_bytes(16), dev)
        rc = L.nbp_recon_curve_update_batch_f32(n, plans, G, lo.ctypes.data, hi.ctypes.data, cell.ctypes.data, cap.ctypes.data, cloud,
                                                capacity, count, seen, d2g, d2n, tot, T, th.ctypes.data, row, bound, _lib.ptr(ws),
                                                ws.numel(), _st())
    _lib.check(rc, "nbp_recon_curve_update_batch_f32")


# ---- held-out view metrics (csrc/nbp_views.hip; the definition of record is utility/view_metrics.py)
def _view_cloud(name, cloud, cloud_rgb, n_dev):
    _nn_points(name, cloud, "cloud")
    _nn_count(name, n_dev, cloud.device)
    if cloud_rgb is not None:
        _nn_points(name, cloud_rgb, "cloud_rgb")
        if cloud_rgb.device != cloud.device or cloud_rgb.shape[0] < cloud.shape[0]:
            raise ValueError(f"{name}: cloud_rgb on the cloud's device with a row for each of its rows expected")


def _view_keys(name, keys, V, H, W, device):
    if (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.device != device or tuple(keys.shape) != (V, H, W)
            or not keys.is_contiguous()):
        raise ValueError(f"{name}: keys must be a contiguous int64 [{V},{H},{W}] tensor on the cloud's device")


def splat_cloud(cloud, cams, H, W, radius=1, n_dev=None, z_far=float("inf"), keys=None, accumulate=False, precheck=True,
                tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """The splat alone -> keys int64 [V,H,W] (the bit pattern of view_metrics.splat's uint64 keys: -1 = empty): per pixel the
    nearest point of cloud [n,3] (n_dev: int64 device counter; rows beyond it are never read) whose (2 radius + 1)^2 footprint
    holds it, cams host [V,12].  keys with accumulate=True: lower an earlier result (a cloud splatted in parts gives the same bits
    as at once, provided each part sits at its own rows of `cloud`: a key's index is the row, so rows outside a part are masked with
    NaN or lie beyond n_dev); precheck=False sends every pixel to the atomic (the same bits; tools/bench_views.py measures both).  No host
    synchronisation."""
    _view_cloud("splat_cloud", cloud, None, n_dev)
    keep, cam_ptr, V = _cam_arg(cams)
    if V < 1:
        raise ValueError("splat_cloud: at least one camera expected")
    if accumulate and keys is None:
        raise ValueError("splat_cloud: accumulate needs the keys of an earlier call")
    if keys is None:
        keys = torch.empty(V, int(H), int(W), dtype=torch.int64, device=cloud.device)
    _view_keys("splat_cloud", keys, V, int(H), int(W), cloud.device)
    with torch.cuda.device(cloud.device):
        rc = _lib.lib().nbp_views_splat_f32(_lib.ptr(cloud), cloud.shape[0], _lib.ptr(n_dev), cam_ptr, V, int(H), int(W), int(radius),
                                            tan_half_fov, float(z_clip), float(z_far), int(bool(accumulate)), int(bool(precheck)),
                                            _lib.ptr(keys), _st())
    _lib.check(rc, "nbp_views_splat_f32")
    return keys


def resolve_views(keys, cloud_rgb=None, n_cloud=None):
    """keys int64 [V,H,W] -> (z [V,H,W] fp32, -1 where empty; rgb [V,H,W,3] = cloud_rgb[index], 0 where empty, or None; index
    [V,H,W] int64, -1 where empty).  n_cloud: rows of the cloud the keys were made from (cloud_rgb's where given)."""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dim() != 3:
        raise RuntimeError("resolve_views: the HIP path needs a cuda tensor [V,H,W] for keys (no CPU fallback)")
    V, H, W = keys.shape
    _view_keys("resolve_views", keys, V, H, W, keys.device)
    if cloud_rgb is not None:
        _nn_points("resolve_views", cloud_rgb, "cloud_rgb")
    if n_cloud is None:
        n_cloud = cloud_rgb.shape[0] if cloud_rgb is not None else (1 << 32) - 2
    if cloud_rgb is not None:
        n_cloud = min(int(n_cloud), cloud_rgb.shape[0])
    z = torch.empty(V, H, W, dtype=torch.float32, device=keys.device)
    index = torch.empty(V, H, W, dtype=torch.int64, device=keys.device)
    rgb = torch.empty(V, H, W, 3, dtype=torch.float32, device=keys.device) if cloud_rgb is not None else None
    with torch.cuda.device(keys.device):
        rc = _lib.lib().nbp_views_resolve_f32(_lib.ptr(keys), _lib.ptr(cloud_rgb), int(n_cloud), V, H, W, _lib.ptr(z), _lib.ptr(rgb),
                                              _lib.ptr(index), _st())
    _lib.check(rc, "nbp_views_resolve_f32")
    return z, rgb, index


def render_cloud(cloud, cloud_rgb, cams, H, W, radius=1, n_dev=None, z_far=float("inf"), keys=None, accumulate=False):
    """Point-splat render of the coloured cloud from cams host [V,12] -> (z [V,H,W] (-1 where empty), rgb [V,H,W,3] | None where
    cloud_rgb is None, index [V,H,W] int64 (-1 where empty)): splat_cloud, then resolve_views.  `keys`: the key buffer to use (it
    holds the splat afterwards); with accumulate=True its earlier content is lowered, not cleared."""
    _view_cloud("render_cloud", cloud, cloud_rgb, n_dev)
    keys = splat_cloud(cloud, cams, H, W, radius, n_dev, z_far, keys, accumulate)
    return resolve_views(keys, cloud_rgb, cloud.shape[0])


def view_stats(keys, cloud_rgb, z_gt, rgb_gt, depth_tolerance=1.0, z_far=float("inf"), n_cloud=None):
    """Resolve + classify + reduce the keys of a splat against the mesh render (z_gt [V,H,W], rgb_gt [V,H,W,3] | None) of the same
    cameras -> raw = (counts int64 [V,6] = n_gt, n_c, n_hit, n_hole, n_leak, n_floater; sums float64 [V,3] = sum |dz|, sum dz^2,
    squared colour error over the hit pixels) on the device; view_metrics.raw_stats is the definition.  Two launches, no
    floating-point atomics (two calls give the same bits), no host synchronisation."""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dim() != 3:
        raise RuntimeError("view_stats: the HIP path needs a cuda tensor [V,H,W] for keys (no CPU fallback)")
    V, H, W = keys.shape
    dev = keys.device
    _view_keys("view_stats", keys, V, H, W, dev)
    if z_gt.dtype != torch.float32 or z_gt.device != dev or tuple(z_gt.shape) != (V, H, W) or not z_gt.is_contiguous():
        raise ValueError("view_stats: z_gt must be a contiguous fp32 [V,H,W] tensor on the keys' device")
    if rgb_gt is not None and (rgb_gt.dtype != torch.float32 or rgb_gt.device != dev or tuple(rgb_gt.shape) != (V, H, W, 3)
                               or not rgb_gt.is_contiguous()):
        raise ValueError("view_stats: rgb_gt must be a contiguous fp32 [V,H,W,3] tensor on the keys' device")
    if cloud_rgb is not None:
        _nn_points("view_stats", cloud_rgb, "cloud_rgb")
    if n_cloud is None:
        n_cloud = cloud_rgb.shape[0] if cloud_rgb is not None else (1 << 32) - 2
    if cloud_rgb is not None:
        n_cloud = min(int(n_cloud), cloud_rgb.shape[0])
    L = _lib.lib()
    counts = torch.empty(V, 6, dtype=torch.int64, device=dev)
    sums = torch.empty(V, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace_for("view_stats", V, lambda: L.nbp_views_stats_workspace_bytes(V), dev)
        rc = L.nbp_views_stats_f64(_lib.ptr(keys), _lib.ptr(cloud_rgb), int(n_cloud), _lib.ptr(z_gt), _lib.ptr(rgb_gt), V, H, W,
                                   float(depth_tolerance), float(z_far), _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(ws), ws.numel(),
                                   _st())
    _lib.check(rc, "nbp_views_stats_f64")
    return counts, sums


class ViewMetrics:
    """Held-out view metrics of a coloured cloud against `mesh`, on the device (utility/view_metrics.py is the definition).  The
    ground truth of the views (cams host [V,12]) is rendered ONCE, here, by the existing rasteriser: depth, and -- for a mesh with
    vertex colours, unless colours=False -- colours with the ambient and contrast settings the rollout's camera renders its own
    frames with, so that both colour images are the same quantity.  evaluate() splats the cloud and reduces; the key buffer
    [V,H,W] belongs to the object.  ground_truth = (z_gt [V,H,W], rgb_gt [V,H,W,3] | None): images rendered elsewhere are taken
    instead (mesh may then be None)."""

    def __init__(self, mesh, cams, H, W, radius=1, depth_tolerance=1.0, z_far=float("inf"), ambient=0.85, contrast=1.0, colours=True,
                 ground_truth=None):
        from . import view_metrics
        keep, _, V = _cam_arg(cams)
        if V < 1:
            raise ValueError("ViewMetrics: at least one camera expected")
        if not 0 <= int(radius) <= view_metrics.MAX_RADIUS:
            raise ValueError(f"ViewMetrics: radius outside 0..{view_metrics.MAX_RADIUS}")
        self.cams, self.V, self.H, self.W = keep.copy(), V, int(H), int(W)
        self.radius, self.depth_tolerance, self.z_far = int(radius), float(depth_tolerance), float(z_far)
        if ground_truth is not None:
            self.z_gt, self.rgb_gt = ground_truth
            self.colours = self.rgb_gt is not None
            if not isinstance(self.z_gt, torch.Tensor) or not self.z_gt.is_cuda or tuple(self.z_gt.shape) != (V, self.H, self.W):
                raise ValueError("ViewMetrics: ground_truth z_gt must be a cuda tensor [V,H,W]")
        else:
            self.colours = bool(colours) and getattr(mesh, "colors", None) is not None
            dev = mesh.verts.device
            self.z_gt = torch.empty(V, self.H, self.W, dtype=torch.float32, device=dev)
            self.rgb_gt = torch.empty(V, self.H, self.W, 3, dtype=torch.float32, device=dev) if self.colours else None
            for v0 in range(0, V, 8):                  # the rasteriser takes 8 cameras per call
                sl = slice(v0, min(v0 + 8, V))
                if self.colours:
                    raster_rgbz(mesh.verts, mesh.faces, mesh.colors, self.cams[sl], self.H, self.W, ambient, contrast,
                                out_z=self.z_gt[sl], out_rgb=self.rgb_gt[sl])
                else:                                  # (the colour render's depth: the same launch without the shading)
                    raster_zface(mesh.verts, mesh.faces, self.cams[sl], self.H, self.W, out_z=self.z_gt[sl])
        self.keys = torch.empty(V, self.H, self.W, dtype=torch.int64, device=self.z_gt.device)
        self.result = None

    def evaluate(self, cloud, cloud_rgb=None, n_dev=None):
        """Enqueues the splat and the statistics on the current stream -> (counts int64 [V,6], sums float64 [V,3]) device tensors;
        no host synchronisation.  cloud_rgb None (or a ground truth without colours): the depth half only.  Kept for raw()."""
        _view_cloud("ViewMetrics.evaluate", cloud, cloud_rgb, n_dev)
        splat_cloud(cloud, self.cams, self.H, self.W, self.radius, n_dev, self.z_far, self.keys)
        rgb = cloud_rgb if self.colours else None
        self.result = view_stats(self.keys, rgb, self.z_gt, self.rgb_gt if rgb is not None else None, self.depth_tolerance,
                                 self.z_far, cloud.shape[0])
        return self.result

    def raw(self):
        """The last evaluation's raw numbers on the host (ONE device -> host copy): view_metrics.pack_raw's float64 rows [V, 9]."""
        if self.result is None:
            raise RuntimeError("ViewMetrics: evaluate() first")
        counts, sums = self.result
        return torch.cat([counts.double(), sums], 1).cpu().numpy()

    def summary(self, options=None):
        from . import view_metrics
        return view_metrics.summarise_raw(self.raw(), options)


# ---- frontier exploration as a policy (csrc/nbp_frontier.hip; the definition is utility/frontier.py)
def _frontier_maps(name, maps6):
    if maps6.dtype != torch.float32 or maps6.dim() != 4 or maps6.shape[1] != 6 or maps6.shape[2] != maps6.shape[3]:
        raise ValueError(f"{name}: maps6 is fp32 [B,6,S,S]")
    return maps6.shape[0], maps6.shape[2]


def frontier_mask(maps6, dilate=2, want_unknown=False):
    """maps6 [B,6,S,S] -> the packed frontier pixels, int64 [B,S,S/64] (bit i of word w of a row = column 64 w + i; read them as
    uint64), or with want_unknown the pair (frontier, unknown).  Four launches."""
    B, S = _frontier_maps("frontier_mask", maps6)
    L = _lib.lib()
    ws = _workspace_for("frontier", (B, S), lambda: L.nbp_frontier_workspace_bytes(B, S), maps6.device)
    bits = torch.empty(B, S, max(S // 64, 1), dtype=torch.int64, device=maps6.device)
    unknown = torch.empty_like(bits) if want_unknown else None
    rc = L.nbp_frontier_mask_u64(_lib.ptr(maps6), B, S, int(dilate), _lib.ptr(bits), _lib.ptr(unknown), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_frontier_mask_u64")
    return (bits, unknown) if want_unknown else bits


def frontier_policy(maps6, radius=24, dilate=2, unknown="free", distance_penalty=0, out=None):
    """maps6 [B,6,S,S] -> (out1 [B,8,V,V], out2 [B,1,S,S]) fp32, V = S / 4: the planner's two inputs from the accumulated maps
    (utility/frontier.py::policy, bit for bit).  out = (out1, out2) to write into.  Five launches, no host synchronisation."""
    B, S = _frontier_maps("frontier_policy", maps6)
    if unknown not in ("free", "obstacle"):
        raise ValueError(f"frontier_policy: unknown must be 'free' or 'obstacle', got {unknown!r}")
    V, dev = S // 4, maps6.device
    if out is None:
        out = (torch.empty(B, 8, V, V, dtype=torch.float32, device=dev), torch.empty(B, 1, S, S, dtype=torch.float32, device=dev))
    out1, out2 = out
    if (out1.dtype, tuple(out1.shape)) != (torch.float32, (B, 8, V, V)) or (out2.dtype, tuple(out2.shape)) != (torch.float32, (B, 1, S, S)):
        raise ValueError("frontier_policy: out is the pair fp32 [B,8,V,V], fp32 [B,1,S,S]")
    L = _lib.lib()
    ws = _workspace_for("frontier", (B, S), lambda: L.nbp_frontier_workspace_bytes(B, S), dev)
    rc = L.nbp_frontier_policy_f32(_lib.ptr(maps6), B, S, int(radius), int(dilate), int(unknown == "obstacle"), int(distance_penalty),
                                   _lib.ptr(out1), _lib.ptr(out2), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_frontier_policy_f32")
    return out1, out2


# ---- ray-cast information gain as a policy (csrc/nbp_infogain.hip; the definition is utility/infogain.py)
def infogain_policy(maps6, radius=24, dilate=2, unknown="free", distance_penalty=0, out=None):
    """maps6 [B,6,S,S] -> (out1 [B,8,V,V], out2 [B,1,S,S]) fp32, V = S / 4: the planner's two inputs from the accumulated maps
    (utility/infogain.py::policy, bit for bit).  out = (out1, out2) to write into.  Five launches, no host synchronisation."""
    B, S = _frontier_maps("infogain_policy", maps6)
    if unknown not in ("free", "obstacle"):
        raise ValueError(f"infogain_policy: unknown must be 'free' or 'obstacle', got {unknown!r}")
    V, dev = S // 4, maps6.device
    if out is None:
        out = (torch.empty(B, 8, V, V, dtype=torch.float32, device=dev), torch.empty(B, 1, S, S, dtype=torch.float32, device=dev))
    out1, out2 = out
    if (out1.dtype, tuple(out1.shape)) != (torch.float32, (B, 8, V, V)) or (out2.dtype, tuple(out2.shape)) != (torch.float32, (B, 1, S, S)):
        raise ValueError("infogain_policy: out is the pair fp32 [B,8,V,V], fp32 [B,1,S,S]")
    L = _lib.lib()
    ws = _workspace_for("infogain", (B, S), lambda: L.nbp_infogain_workspace_bytes(B, S), dev)
    rc = L.nbp_infogain_policy_f32(_lib.ptr(maps6), B, S, int(radius), int(dilate), int(unknown == "obstacle"), int(distance_penalty),
                                   _lib.ptr(out1), _lib.ptr(out2), _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_infogain_policy_f32")
    return out1, out2


def infogain_visible(maps6, radius=24, dilate=2, cells=()):
    """maps6 [B,6,S,S], cells [n,3] = (b, g0, g1) on the host -> the visible masks of those cells, int64 [n, 2 radius + 1] on the
    device (bit dx + radius of word dy + radius = pixel (4 g0 + dy, 4 g1 + dx) is visible from the cell; read them as uint64):
    utility/infogain.py::visible, packed.  To locate a gain mismatch."""
    import numpy as np
    B, S = _frontier_maps("infogain_visible", maps6)
    cells = np.ascontiguousarray(np.asarray(cells, np.int32).reshape(-1, 3))
    n, R = len(cells), int(radius)
    out = torch.empty(n, 2 * max(R, 0) + 1, dtype=torch.int64, device=maps6.device)
    if n == 0:
        return out
    L = _lib.lib()
    ws = _workspace_for("infogain", (B, S), lambda: L.nbp_infogain_workspace_bytes(B, S), maps6.device)
    rc = L.nbp_infogain_visible_u64(_lib.ptr(maps6), B, S, R, int(dilate), cells.ctypes.data, n, _lib.ptr(out),
                                    _lib.ptr(ws), ws.numel(), _st())
    _lib.check(rc, "nbp_infogain_visible_u64")
    return out


# ---- TSDF fusion of depth frames (csrc/nbp_tsdf.hip; the definition is utility/tsdf.py)
def _tsdf_volume(name, vol):
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a cuda tensor for the volume (no CPU fallback)")
    if vol.dim() != 4 or vol.shape[3] != 2 or vol.dtype != torch.int32 or not vol.is_contiguous() or vol.numel() == 0:
        raise ValueError(f"{name}: the volume must be a contiguous int32 [nx,ny,nz,2] tensor")
    return tuple(int(d) for d in vol.shape[:3])


def _tsdf_frames(name, depth, device, H, W):
    """depth: fp32 [n,H,W] or [H,W] (consecutive frames), or a list of [H,W] tensors / device pointers (then H and W are needed)
    -> (base pointer | None, pointer list | None, n, H, W)."""
    if isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise RuntimeError(f"{name}: the HIP path needs cuda tensors for the frames (no CPU fallback)")
        if depth.dtype != torch.float32 or depth.dim() not in (2, 3) or not depth.is_contiguous() or depth.device != device:
            raise ValueError(f"{name}: frames are contiguous fp32 [n,H,W] (or [H,W]) on the volume's device")
        return depth.data_ptr(), None, (depth.shape[0] if depth.dim() == 3 else 1), int(depth.shape[-2]), int(depth.shape[-1])
    ptrs = []
    for t in depth:
        if isinstance(t, int):
            ptrs.append(t)
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: the HIP path needs cuda tensors for the frames (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.device != device or (H is not None and tuple(t.shape) != (H, W)):
            raise ValueError(f"{name}: frames are contiguous fp32 [H,W] tensors of one shape on the volume's device")
        H, W = int(t.shape[0]), int(t.shape[1])
        ptrs.append(t.data_ptr())
    if ptrs and (H is None or W is None):
        raise ValueError(f"{name}: frames given as pointers need H and W")
    return None, ptrs, len(ptrs), H, W


def tsdf_integrate(vol, lo, voxel, depth, cams, trunc, max_depth, H=None, W=None, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """Integrates n depth frames into ONE volume int32 [nx,ny,nz,2] (in place; tsdf.integrate frame by frame, bit for bit, in any
    order).  depth: fp32 [n,H,W] / [H,W], or a list of [H,W] tensors or device pointers (with H, W); cams host [n,12].  One launch
    per 4 frames, no host synchronisation.  Returns vol."""
    dims = _tsdf_volume("tsdf_integrate", vol)
    base, ptrs, n, H, W = _tsdf_frames("tsdf_integrate", depth, vol.device, H, W)
    keep, cam_ptr, n_cams = _cam_arg(cams)
    if n < 1 or n_cams != n:
        raise ValueError(f"tsdf_integrate: {n} frames with {n_cams} cameras")
    lo3 = (C.c_float * 3)(*[float(v) for v in lo])
    table = None if ptrs is None else (C.c_void_p * n)(*ptrs)
    with torch.cuda.device(vol.device):
        rc = _lib.lib().nbp_tsdf_integrate_f32(_lib.ptr(vol), lo3, float(voxel), *dims, base, table, n, cam_ptr, H, W, float(tan_half_fov),
                                               float(z_clip), float(trunc), float(max_depth), _st())
    _lib.check(rc, "nbp_tsdf_integrate_f32")
    return vol


def tsdf_integrate_batch(items, H=None, W=None, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """tsdf_integrate for several volumes in ONE launch.  items = [(vol, lo, voxel, trunc, max_depth, frames, cams host [F,12])]
    (TSDFVolume.item makes them): per item its own volume and geometry and 1 to 4 frames, each an [H,W] fp32 tensor or a device
    pointer (then H and W are needed), which need not be adjacent in memory.  Each volume gets the bits of a call of its own.  More
    than 12 items go in chunks of 12."""
    import numpy as np
    if len(items) > 12:
        for i in range(0, len(items), 12):
            tsdf_integrate_batch(items[i:i + 12], H, W, tan_half_fov, z_clip)
        return
    n = len(items)
    if n == 0:
        return
    dev = items[0][0].device if isinstance(items[0][0], torch.Tensor) else None
    vols, frames, nf = (C.c_void_p * n)(), (C.c_void_p * (4 * n))(), (C.c_int * n)()
    lo, voxel, dims = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.int32)
    trunc, max_depth, cams = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 4, 12), np.float32)
    for i, (vol, lo_i, voxel_i, trunc_i, max_depth_i, fr, cam) in enumerate(items):
        dims[i] = _tsdf_volume("tsdf_integrate_batch", vol)
        if vol.device != dev:
            raise ValueError("tsdf_integrate_batch: the items of one call on one device expected")
        _, ptrs, k, H, W = _tsdf_frames("tsdf_integrate_batch", list(fr), dev, H, W)
        cam = np.asarray(cam, np.float32).reshape(-1, 12)
        if not 1 <= k <= 4 or cam.shape[0] != k:
            raise ValueError("tsdf_integrate_batch: an item has 1 to 4 frames and as many cameras")
        vols[i], nf[i], lo[i], voxel[i], trunc[i], max_depth[i] = vol.data_ptr(), k, lo_i, voxel_i, trunc_i, max_depth_i
        cams[i, :k] = cam
        for f in range(k):
            frames[4 * i + f] = ptrs[f]
    with torch.cuda.device(dev):
        rc = _lib.lib().nbp_tsdf_integrate_batch_f32(n, vols, lo.ctypes.data, voxel.ctypes.data, dims.ctypes.data, trunc.ctypes.data,
                                                     max_depth.ctypes.data, nf, frames, cams.ctypes.data, int(H), int(W),
                                                     float(tan_half_fov), float(z_clip), _st())
    _lib.check(rc, "nbp_tsdf_integrate_batch_f32")


def tsdf_extract(vol, lo, voxel, min_weight=1, out=None):
    """The fused surface cloud of a volume, in tsdf.extract's order -> (points fp32 [.,3], total int64 [1] on the device).  `out`
    given (fp32 [capacity,3]): its first min(total, capacity) rows are written and nothing beyond them, with no host
    synchronisation.  out=None: the points are counted first, the total is read back (the ONE host synchronisation of this path:
    it belongs to the evaluation at a rollout's end) and exactly total rows are returned."""
    dims = _tsdf_volume("tsdf_extract", vol)
    n_vox = dims[0] * dims[1] * dims[2]
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != vol.device or out.dtype != torch.float32
                            or out.dim() != 2 or out.shape[1] != 3 or not out.is_contiguous()):
        raise ValueError("tsdf_extract: out must be a contiguous fp32 [capacity,3] tensor on the volume's device")
    L = _lib.lib()
    lo3 = (C.c_float * 3)(*[float(v) for v in lo])
    total = torch.zeros(1, dtype=torch.int64, device=vol.device)

    def call(points, capacity):
        with torch.cuda.device(vol.device):
            ws = _workspace_for("tsdf_extract", n_vox, lambda: L.nbp_tsdf_extract_workspace_bytes(n_vox), vol.device)
            rc = L.nbp_tsdf_extract_f32(_lib.ptr(vol), lo3, float(voxel), *dims, int(min_weight), _lib.ptr(points), capacity,
                                        _lib.ptr(total), _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_tsdf_extract_f32")

    if out is not None:
        call(out if out.shape[0] else None, out.shape[0])
        return out, total
    call(None, 0)
    n = int(total.item())
    out = torch.empty(n, 3, dtype=torch.float32, device=vol.device)
    if n:
        call(out, n)
    return out, total


def tsdf_stats(vol, min_weight=1):
    """int64 [2] on the device: the voxels with W > 0, the usable voxels (tsdf.stats).  Two launches, no host synchronisation."""
    dims = _tsdf_volume("tsdf_stats", vol)
    L = _lib.lib()
    counts = torch.empty(2, dtype=torch.int64, device=vol.device)
    with torch.cuda.device(vol.device):
        ws = _workspace_for("tsdf_stats", 0, L.nbp_tsdf_stats_workspace_bytes, vol.device)
        rc = L.nbp_tsdf_stats_i64(_lib.ptr(vol), dims[0] * dims[1] * dims[2], int(min_weight), _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
                                  _st())
    _lib.check(rc, "nbp_tsdf_stats_i64")
    return counts


class TSDFVolume:
    """The TSDF volume of one rollout on the device (utility/tsdf.py is the definition): int32 [nx,ny,nz,2] over bbox = (lo, hi) of
    the GT grown by trunc.  spec: tsdf.option_spec's dict with max_depth resolved (tsdf.resolved_options); it is `.options`.
    `frames` counts the frames integrated so far (on the host)."""

    def __init__(self, bbox, spec, device):
        from . import tsdf
        spec = tsdf.option_spec(spec)
        if spec is None or "max_depth" not in spec:
            raise ValueError("TSDFVolume: a spec with max_depth is needed (tsdf.resolved_options; None means off: nothing to build)")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TSDFVolume: the HIP path needs a cuda device (no CPU fallback)")
        self.options = spec
        lo, dims = tsdf.volume_geometry(bbox, spec)
        self.lo, self.dims = [float(v) for v in lo], tuple(int(d) for d in dims)
        self.voxel, self.trunc, self.max_depth, self.min_weight = spec["voxel"], spec["trunc"], spec["max_depth"], spec["min_weight"]
        self.vol = torch.zeros(*self.dims, 2, dtype=torch.int32, device=device)
        self.frames = 0

    def reset(self):
        """An empty volume again.  Enqueue-only."""
        self.vol.zero_()
        self.frames = 0

    def integrate(self, depth, cams, H=None, W=None):
        """`depth` (tsdf_integrate's forms) with cams host [n,12] into the volume: one call, no host synchronisation."""
        tsdf_integrate(self.vol, self.lo, self.voxel, depth, cams, self.trunc, self.max_depth, H, W)
        self.frames += len(cams)

    def item(self, frames, cams):
        """The arguments of tsdf_integrate_batch for 1 to 4 frames (a list of [H,W] tensors or device pointers) of this volume.
        Making an item counts its frames: an item is made to be launched."""
        self.frames += len(cams)
        return (self.vol, self.lo, self.voxel, self.trunc, self.max_depth, frames, cams)

    def extract(self):
        """(points fp32 [n,3] on the device, n): the fused surface cloud.  Reads the count back (one host synchronisation)."""
        points, total = tsdf_extract(self.vol, self.lo, self.voxel, self.min_weight)
        return points, points.shape[0]

    def stats(self):
        """{"observed_voxels", "usable_voxels"} on the host (one device -> host copy)."""
        observed, usable = tsdf_stats(self.vol, self.min_weight).tolist()
        return {"observed_voxels": int(observed), "usable_voxels": int(usable)}

    def mesh(self):
        """(verts fp32 [V,3], faces int32 [F,3]) on the device: the fused mesh (utility/tsdf_mesh.py).  Reads the two counts back
        (one host synchronisation)."""
        verts, faces, _ = tsdf_mesh(self.vol, self.lo, self.voxel, self.min_weight)
        return verts, faces


# ---- the fused mesh (csrc/nbp_tsdf_mesh.hip; the definition is utility/tsdf_mesh.py)
def _mesh_out(name, what, t, dtype, width, device):
    if t is None:
        return 0
    shape_ok = isinstance(t, torch.Tensor) and (t.dim() == 2 and t.shape[1] == 3 if width == 3 else t.dim() == 1)
    if not shape_ok or t.device != device or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} [capacity{',3' if width == 3 else ''}] tensor on the volume's device")
    return t.shape[0]


def tsdf_mesh(vol, lo, voxel, min_weight=1, verts_out=None, faces_out=None, area2_out=None):
    """The surface-nets mesh of a volume (tsdf_mesh.mesh, bit for bit) -> (verts fp32 [.,3], faces int32 [.,3], totals int64 [2] on
    the device = the numbers of vertices and faces).  With verts_out (fp32 [capacity,3]) or faces_out (int32 [capacity,3]; area2_out
    fp32 of as many rows beside it receives each face's squared area) given: their first min(total, capacity) rows are written and
    nothing beyond them, with no host synchronisation; a buffer not given is not produced (None).  With none given: counted first,
    the two totals read back once (the ONE host synchronisation of this path: it belongs to the evaluation at a rollout's end) and
    exactly-sized tensors returned."""
    dims = _tsdf_volume("tsdf_mesh", vol)
    n_vox = dims[0] * dims[1] * dims[2]
    dev = vol.device
    vcap = _mesh_out("tsdf_mesh", "verts_out", verts_out, torch.float32, 3, dev)
    fcap = _mesh_out("tsdf_mesh", "faces_out", faces_out, torch.int32, 3, dev)
    acap = _mesh_out("tsdf_mesh", "area2_out", area2_out, torch.float32, 1, dev)
    if area2_out is not None and (faces_out is None or acap != fcap):
        raise ValueError("tsdf_mesh: area2_out goes with a faces_out of as many rows")
    L = _lib.lib()
    lo3 = (C.c_float * 3)(*[float(v) for v in lo])
    totals = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(verts, faces, area2):
        nv, nf = (0 if verts is None else verts.shape[0]), (0 if faces is None else faces.shape[0])
        with torch.cuda.device(dev):
            ws = _workspace_for("tsdf_mesh", n_vox, lambda: L.nbp_tsdf_mesh_workspace_bytes(n_vox), dev)
            rc = L.nbp_tsdf_mesh_f32(_lib.ptr(vol), lo3, float(voxel), *dims, int(min_weight), _lib.ptr(verts) if nv else None, nv,
                                     _lib.ptr(faces) if nf else None, _lib.ptr(area2) if nf and area2 is not None else None, nf,
                                     _lib.ptr(totals), _lib.ptr(ws), ws.numel(), _st())
        _lib.check(rc, "nbp_tsdf_mesh_f32")

    if verts_out is not None or faces_out is not None:
        call(verts_out, faces_out, area2_out)
        return verts_out, faces_out, totals
    call(None, None, None)
    nv, nf = (int(v) for v in totals.tolist())
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    if nv:
        call(verts, faces, None)
    return verts, faces, totals


class FusedMeshMetrics:
    """The fused mesh of a TSDFVolume against the GT, on the device (utility/tsdf_mesh.py::reference_raw is the definition).
    Completeness: GT sample -> fused SURFACE, exact point-to-triangle distances through a MeshPlan over the fused mesh, inside the
    volume's bounds grown by `cap` (tsdf_mesh.volume_box).  Accuracy: the fused mesh's vertices -> GT mesh, through
    `gt_mesh_metrics`, the rollout's SurfaceMetrics, which must have these thresholds and this cap.  Area: recon_stats over the
    faces' squared areas, whose "sum of sqrt" is the area in fixed-order float64.  gt fp32 [G,3] on the device."""

    def __init__(self, gt, gt_mesh_metrics, thresholds=None, cap=5.0, cell=1.0):
        from . import surface_metrics
        thresholds = surface_metrics.DEFAULT_THRESHOLDS if thresholds is None else thresholds
        self.thresholds, self.cap, self.cell = surface_metrics.check_options(thresholds, cap, cell)
        _nn_points("FusedMeshMetrics", gt, "gt")
        if gt.shape[0] < 1:
            raise ValueError("FusedMeshMetrics: an empty GT surface")
        if tuple(gt_mesh_metrics.thresholds) != self.thresholds or gt_mesh_metrics.cap != self.cap:
            raise ValueError("FusedMeshMetrics: gt_mesh_metrics was built with other thresholds or another cap")
        self.gt, self.G, self.gt_mesh_metrics = gt, gt.shape[0], gt_mesh_metrics
        self.row = self.mesh = None         # the last evaluation: its raw row, and (verts, faces) on the device

    def evaluate(self, volume):
        """Meshes `volume` (a TSDFVolume) and measures it -> tsdf_mesh.pack_raw's float64 vector on the host (kept for raw() /
        summary()).  Synchronises with the host: the mesh's counts, the plan's build and the results are read back."""
        from . import tsdf_mesh as definition
        dev = volume.vol.device
        counts = tsdf_mesh(volume.vol, volume.lo, volume.voxel, volume.min_weight)[2]
        _, crossings = tsdf_extract(volume.vol, volume.lo, volume.voxel, volume.min_weight,
                                    out=torch.empty(0, 3, dtype=torch.float32, device=dev))
        nv, nf, nc = (int(v) for v in torch.cat([counts, crossings]).tolist())
        verts = torch.empty(max(nv, 1), 3, dtype=torch.float32, device=dev)
        faces = torch.empty(max(nf, 1), 3, dtype=torch.int32, device=dev)
        area2 = torch.empty(max(nf, 1), dtype=torch.float32, device=dev)
        if nv:
            tsdf_mesh(volume.vol, volume.lo, volume.voxel, volume.min_weight, verts, faces, area2)
        if nf:
            lo, hi = definition.volume_box(volume.lo, volume.voxel, volume.dims, self.cap)
            plan = MeshPlan(verts[:nv], faces[:nf], (lo.tolist(), hi.tolist()), self.cell)
            comp = recon_stats(plan.dist2(self.gt, self.cap), self.thresholds)
            area = recon_stats(area2[:nf], self.thresholds)[0][:1]
            flat = torch.cat([comp[0], comp[1].double(), area]).cpu().numpy()
            T = len(self.thresholds)
            comp_sums, comp_counts, area = flat[0:2], flat[2:2 + T], float(flat[2 + T])
        else:                           # no face, no plan: the definition's row, every GT point `cap` away
            comp_sums, comp_counts = definition.cap_row(self.G, self.thresholds, self.cap)
            area = 0.0
        if not nv:
            verts.zero_()                # (one dummy row; the count says that none is valid)
        self.gt_mesh_metrics.evaluate(verts, torch.full((1,), nv, dtype=torch.int64, device=dev))
        self.row = definition.pack_raw(nv, nf, nf // 2, nc, area, comp_sums, comp_counts, self.G, self.gt_mesh_metrics.raw())
        self.mesh = (verts[:nv], faces[:nf])
        return self.row

    def raw(self):
        if self.row is None:
            raise RuntimeError("FusedMeshMetrics: evaluate() first")
        return self.row

    def summary(self, options=None):
        """The last evaluation as tsdf_mesh.summarise_raw's dict (`options`: the volume's, for the block's "options")."""
        from . import tsdf_mesh as definition
        return definition.summarise_raw(self.raw(), {"thresholds": self.thresholds, "cap": self.cap, "cell": self.cell}, options)
