"""The size functions of the carved workspaces (csrc/nbp_carve.h), on the host: every *_bytes function is its layout run dry, and
may only have GROWN against the hand-written sums it replaced -- by rounding, so by at most 256 bytes per buffer of its layout.
PARENT holds what the commit before the layouts returned for each case (recorded from a build of that commit); a refusal (0)
stays a refusal, and the forward's three functions, whose allocation sequence did not change, return exactly what they did."""
import ctypes as C

import pytest

from nextbestpath_amd import _lib

F3 = C.c_float * 3
BOX = ((0.0, 0.0, 0.0), (4.0, 3.0, 5.0))                 # a small box that divides into a few hundred cells
POINT = ((1.0, 2.0, 3.0), (1.0, 2.0, 3.0))               # hi == lo: one grid cell on every axis (shell-walk grids)
ROOM = ((-16.0, -1.0, -16.0), (16.0, 7.0, 16.0))         # a scene-sized box for the workload's shapes
H, W = 256, 456                                          # the default config's image


def _box(fn, box, *rest):
    return fn(F3(*box[0]), F3(*box[1]), *rest)


def _scene(fn, box, grid, *rest):
    return fn((C.c_float * 6)(*box[0], *box[1]), (C.c_int * 3)(*grid), *rest)


def _bins(fn, lo, hi, capacity):
    return fn((C.c_float * 2)(*lo), (C.c_float * 2)(*hi), capacity)


def _plain(fn, *args):
    return fn(*args)


# name -> (how to call it, buffers in its layout; None: exact)
FUNCS = {
    "nbp_unproject_workspace_bytes": (_plain, 2),
    "nbp_raster_workspace_bytes": (_plain, 3),
    "nbp_raster_rgb_workspace_bytes": (_plain, 5),
    "nbp_coverage_workspace_bytes": (_box, 7),
    "nbp_coverage_plan_bytes": (_box, 3),
    "nbp_coverage_plan_workspace_bytes": (_box, 4),
    "nbp_scene_fill_workspace_bytes": (_scene, 13),
    "nbp_scene_coverage_workspace_bytes": (_scene, 6),
    "nbp_nn_plan_bytes": (_box, 2),
    "nbp_nn_plan_workspace_bytes": (_box, 4),
    "nbp_nn_dist2_workspace_bytes": (_box, 6),
    "nbp_mesh_plan_bytes": (_box, 2),
    "nbp_mesh_plan_workspace_bytes": (_box, 2),
    "nbp_cloud_bins_bytes": (_bins, 5),
    "nbp_forward_workspace_bytes": (_plain, None),
    "nbp_forward_workspace_bytes_bf16": (_plain, None),
    "nbp_forward_workspace_bytes_split": (_plain, None),
}

NAN = float("nan")
# (function, arguments, what the parent commit returned)
PARENT = [
    # ---- un-projection (n_frames, H, W): smallest, the fast path's and the slow path's small frames, the workload's, refused
    ("nbp_unproject_workspace_bytes", (1, 2, 2), 784),
    ("nbp_unproject_workspace_bytes", (1, 8, 12), 1152),
    ("nbp_unproject_workspace_bytes", (4, 8, 12), 2304),
    ("nbp_unproject_workspace_bytes", (4, 7, 9), 1776),
    ("nbp_unproject_workspace_bytes", (4, 32, 32), 17152),
    ("nbp_unproject_workspace_bytes", (4, 64, 32), 33536),         # exactly one 2048-pixel chunk
    ("nbp_unproject_workspace_bytes", (8, 64, 33), 68352),         # two of them, eight frames
    ("nbp_unproject_workspace_bytes", (4, 456, 256), 1869312),
    ("nbp_unproject_workspace_bytes", (4, H, W), 1869312),
    ("nbp_unproject_workspace_bytes", (0, 8, 8), 0),
    ("nbp_unproject_workspace_bytes", (1, 1, 8), 0),
    ("nbp_unproject_workspace_bytes", (1, 8, 1), 0),
    # ---- rasteriser (n_faces, n_frames, H, W[, bin_cap])
    ("nbp_raster_workspace_bytes", (1, 1, 1, 1, 0), 1280),
    ("nbp_raster_workspace_bytes", (12, 4, 32, 32, 0), 3584),
    ("nbp_raster_workspace_bytes", (13, 4, 7, 9, 0), 3840),
    ("nbp_raster_workspace_bytes", (13, 2, 24, 40, 0), 2304),
    ("nbp_raster_workspace_bytes", (5000, 4, H, W, 0), 6081024),
    ("nbp_raster_workspace_bytes", (0, 1, 8, 8, 0), 0),
    ("nbp_raster_workspace_bytes", (1, 0, 8, 8, 0), 0),
    ("nbp_raster_workspace_bytes", (1, 1, 0, 8, 0), 0),
    ("nbp_raster_rgb_workspace_bytes", (1, 1, 1, 1), 1792),
    ("nbp_raster_rgb_workspace_bytes", (12, 4, 32, 32), 36608),
    ("nbp_raster_rgb_workspace_bytes", (13, 4, 7, 9), 6144),
    ("nbp_raster_rgb_workspace_bytes", (5000, 4, H, W), 9816832),
    ("nbp_raster_rgb_workspace_bytes", (1, 1, 8, 0), 0),
    # ---- coverage (box, threshold, sample_k | G)
    ("nbp_coverage_workspace_bytes", (BOX, 1.0, 100), 7424),
    ("nbp_coverage_workspace_bytes", (BOX, 1.0, 1), 4864),
    ("nbp_coverage_workspace_bytes", (BOX, 0.3, 13), 31232),
    ("nbp_coverage_workspace_bytes", (ROOM, 0.25, 100000), 8006912),
    ("nbp_coverage_workspace_bytes", (BOX, 0.0, 100), 0),
    ("nbp_coverage_workspace_bytes", (BOX, 1.0, 0), 0),
    ("nbp_coverage_plan_bytes", (BOX, 1.0, 50), 3072),
    ("nbp_coverage_plan_bytes", (BOX, 1.0, 1), 2304),
    ("nbp_coverage_plan_bytes", (BOX, 0.3, 13), 15616),
    ("nbp_coverage_plan_bytes", (ROOM, 0.25, 50000), 3403008),
    ("nbp_coverage_plan_bytes", (BOX, 1.0, 0), 0),
    ("nbp_coverage_plan_bytes", (BOX, NAN, 50), 0),
    ("nbp_coverage_plan_workspace_bytes", (BOX, 1.0, 50), 2560),
    ("nbp_coverage_plan_workspace_bytes", (BOX, 1.0, 1), 2560),
    ("nbp_coverage_plan_workspace_bytes", (BOX, 0.3, 13), 15616),
    ("nbp_coverage_plan_workspace_bytes", (ROOM, 0.25, 50000), 2803968),
    ("nbp_coverage_plan_workspace_bytes", (BOX, -1.0, 50), 0),
    # ---- scene store (box, grid, capacity, n_pts_max, resolution | capacity_rec, epsilon)
    ("nbp_scene_fill_workspace_bytes", (BOX, (1, 1, 1), 1, 1, 1.0), 6400),
    ("nbp_scene_fill_workspace_bytes", (BOX, (2, 2, 2), 16, 100, 0.5), 19200),
    ("nbp_scene_fill_workspace_bytes", (BOX, (3, 1, 5), 13, 77, 0.3), 43264),
    ("nbp_scene_fill_workspace_bytes", (ROOM, (5, 3, 5), 20000, 100000, 0.05), 90086144),
    ("nbp_scene_fill_workspace_bytes", (BOX, (2, 0, 2), 16, 100, 0.5), 0),
    ("nbp_scene_fill_workspace_bytes", (BOX, (2, 2, 2), 0, 100, 0.5), 0),
    ("nbp_scene_fill_workspace_bytes", (BOX, (2, 2, 2), 16, 0, 0.5), 0),
    ("nbp_scene_fill_workspace_bytes", (BOX, (2, 2, 2), 16, 100, 0.0), 0),
    ("nbp_scene_coverage_workspace_bytes", (BOX, (1, 1, 1), 1, 1.0), 4608),
    ("nbp_scene_coverage_workspace_bytes", (BOX, (2, 2, 2), 16, 0.5), 14592),
    ("nbp_scene_coverage_workspace_bytes", (ROOM, (5, 3, 5), 20000, 0.05), 70084096),
    ("nbp_scene_coverage_workspace_bytes", (BOX, (2, 2, 2), 0, 0.5), 0),
    ("nbp_scene_coverage_workspace_bytes", (BOX, (41, 40, 40), 16, 0.5), 0),
    # ---- shell-walk grids (box, cell, T | F)
    ("nbp_nn_plan_bytes", (BOX, 1.0, 50), 1792),
    ("nbp_nn_plan_bytes", (POINT, 1.0, 0), 768),
    ("nbp_nn_plan_bytes", (BOX, 0.3, 13), 10240),
    ("nbp_nn_plan_bytes", (ROOM, 0.25, 50000), 2996992),
    ("nbp_nn_plan_bytes", (BOX, 1.0, -1), 0),
    ("nbp_nn_plan_bytes", (BOX, 0.0, 50), 0),
    ("nbp_nn_plan_workspace_bytes", (BOX, 1.0, 50), 1536),
    ("nbp_nn_plan_workspace_bytes", (POINT, 1.0, 0), 1280),
    ("nbp_nn_plan_workspace_bytes", (BOX, 0.3, 13), 10752),
    ("nbp_nn_plan_workspace_bytes", (ROOM, 0.25, 50000), 2598144),
    ("nbp_nn_plan_workspace_bytes", (BOX, 1.0, 1 << 31), 0),
    ("nbp_nn_dist2_workspace_bytes", (BOX, 1.0, 50), 3328),
    ("nbp_nn_dist2_workspace_bytes", (POINT, 1.0, 1), 2048),
    ("nbp_nn_dist2_workspace_bytes", (BOX, 0.3, 13), 20992),
    ("nbp_nn_dist2_workspace_bytes", (ROOM, 0.25, 50000), 5595136),
    ("nbp_nn_dist2_workspace_bytes", ((BOX[1], BOX[0]), 1.0, 50), 0),
    ("nbp_mesh_plan_bytes", (BOX, 1.0, 20), 1792),
    ("nbp_mesh_plan_bytes", (POINT, 1.0, 1), 768),
    ("nbp_mesh_plan_bytes", (BOX, 0.3, 13), 10752),
    ("nbp_mesh_plan_bytes", (ROOM, 0.25, 5000), 2437120),
    ("nbp_mesh_plan_bytes", (BOX, 1.0, -1), 0),
    ("nbp_mesh_plan_workspace_bytes", (BOX, 1.0), 1024),
    ("nbp_mesh_plan_workspace_bytes", (POINT, 1.0), 768),
    ("nbp_mesh_plan_workspace_bytes", (ROOM, 0.25), 2197760),
    ("nbp_mesh_plan_workspace_bytes", (BOX, 1e-6), 0),
    # ---- cloud bins (lo_xz, hi_xz, capacity)
    ("nbp_cloud_bins_bytes", ((0.0, 0.0), (40.0, 30.0), 100000), 10030336),
    ("nbp_cloud_bins_bytes", ((3.0, 4.0), (3.0, 4.0), 1), 2065408),            # an extent of zero
    ("nbp_cloud_bins_bytes", ((-16.0, -16.0), (16.0, 16.0), 3000000), 43385088),
    ("nbp_cloud_bins_bytes", ((0.0, 0.0), (40.0, 30.0), 0), 0),
    ("nbp_cloud_bins_bytes", ((0.0, 0.0), (-1.0, 30.0), 1000), 0),
    # ---- the network's forward (B, S): exact
    ("nbp_forward_workspace_bytes", (1, 256), 276300032),
    ("nbp_forward_workspace_bytes", (1, 16), 1997056),
    ("nbp_forward_workspace_bytes", (2, 64), 47120640),
    ("nbp_forward_workspace_bytes", (0, 64), 0),
    ("nbp_forward_workspace_bytes", (1, 24), 0),
    ("nbp_forward_workspace_bytes_bf16", (1, 256), 138150144),
    ("nbp_forward_workspace_bytes_bf16", (1, 16), 998656),
    ("nbp_forward_workspace_bytes_bf16", (2, 64), 31949056),
    ("nbp_forward_workspace_bytes_bf16", (1, 8), 0),
    ("nbp_forward_workspace_bytes_split", (1, 256), 276332800),
    ("nbp_forward_workspace_bytes_split", (1, 16), 2029824),
    ("nbp_forward_workspace_bytes_split", (2, 64), 47153408),
    ("nbp_forward_workspace_bytes_split", (1, 0), 0),
]


def query(L, name, args):
    how, _ = FUNCS[name]
    return int(how(getattr(L, name), *args))


def test_every_size_function_has_cases():
    assert {name for name, _, _ in PARENT} == set(FUNCS)
    for name in FUNCS:
        values = [want for n, _, want in PARENT if n == name]
        assert 0 in values and any(v > 0 for v in values), name          # refused and accepted arguments both


@pytest.mark.parametrize("name,args,parent", PARENT, ids=[f"{n[4:]}-{i}" for i, (n, _, _) in enumerate(PARENT)])
def test_size_is_the_parents_or_grew_by_rounding_only(name, args, parent):
    got = query(_lib.lib(), name, args)
    buffers = FUNCS[name][1]
    if parent == 0 or buffers is None:
        assert got == parent
    else:
        assert parent <= got <= parent + 256 * buffers, (got, parent)
