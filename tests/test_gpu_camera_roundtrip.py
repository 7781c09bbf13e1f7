"""GPU: the camera's one definition (csrc/nbp_camera.h) taken round: every pixel of a depth frame is un-projected
(hipops.unproject_append, gathering_factor = 1), the points are splatted with radius 0 (hipops.splat_cloud) and each must land on
the pixel it came from; hipops.points_in_fov must accept all of them.  Un-projection, projection and the field-of-view bounds
share the NDC-tables convention: were one of them to drift to the rasteriser's pixel centres (or to another rounding), points
would land on a neighbour or fall outside the corners.

Frames of 6x10, 10x6 and 7x5 (the conventions scale by min(H, W): 5x7 would be no further case), one camera that looks along no
axis of the world (eight of the rotation's nine entries are non-zero) from a translated place.  The round trip is exact in real
arithmetic only; in fp32 a corner pixel's NDC may come back one ulp outside the tables' corner.  So the depths are CHOSEN: drawn per pixel and drawn again until the numpy definitions alone
(oracle/camera.py, view_metrics.project) take every pixel round, which the first test checks without a GPU.  The device then has
to agree with them, pixel for pixel."""
import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import view_metrics as vm
from oracle import camera as oc
from oracle import sampling

f32 = np.float32
SHAPES = [(6, 10), (10, 6), (7, 5)]
FOV_RANGE, SEED = 70.0, 5
R, T = oc.look_at_RT((1.5, -0.7, 2.2), (4.0, 1.1, -3.0))


def _round_trip_ok(depth):
    """Per pixel: the definitions project the un-projected pixel onto itself, and inside the field of view."""
    H, W = depth.shape
    pts = oc.unproject(depth, R, T)
    ok, row, col, _ = vm.project(pts, R, T, H, W)
    rows, cols = np.divmod(np.arange(H * W), W)
    return (ok & (row == rows) & (col == cols) & oc.points_in_fov(pts, R, T, H, W, FOV_RANGE)).reshape(H, W)


def _frame(H, W):
    rng = np.random.default_rng(100 * H + W)
    depth = rng.uniform(2.0, 10.0, (H, W)).astype(f32)
    for _ in range(64):
        bad = ~_round_trip_ok(depth)
        if not bad.any():
            return depth
        depth[bad] = rng.uniform(2.0, 10.0, int(bad.sum())).astype(f32)
    raise AssertionError("no depths found that the definitions take round")


@pytest.mark.parametrize("H,W", SHAPES)
def test_definitions_round_trip_every_pixel(H, W):
    assert np.count_nonzero(np.abs(R) > 0.05) == 8 and np.all(np.abs(T) > 0.2)      # about no axis of the world, and translated
    depth = _frame(H, W)
    assert depth.shape == (H, W) and np.all(depth > vm.Z_CLIP) and np.all(depth < FOV_RANGE)
    assert np.all(_round_trip_ok(depth))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_unprojected_pixels_splat_onto_themselves_and_lie_in_the_fov(hip, H, W):
    from nextbestpath_amd.utility import hipops
    depth = _frame(H, W)
    n = H * W
    cams = hipops.cams12(R[None], T[None])
    cloud = torch.full((n + 3, 3), float("nan"), device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = hipops.unproject_append(torch.from_numpy(depth[None]).cuda(), None, cams, cloud, count, gathering_factor=1.0,
                                     fov_range=FOV_RANGE, seed=SEED).clone()
    assert int(count.item()) == n and counts.cpu().tolist() == [[n, n]]
    # row i of the cloud is pixel sel[i] (oracle/camera.py::partial_point_cloud's order), bit for bit the definition's point
    sel = sampling.perm_index(np.arange(n), n, (SEED + 0x632BE5AB) & sampling.M32)
    assert sorted(sel.tolist()) == list(range(n))
    want = oc.unproject(depth, R, T)[sel]
    got = cloud[:n].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    keys = hipops.splat_cloud(cloud[:n], cams, H, W, radius=0)
    _, _, index = hipops.resolve_views(keys, None, n_cloud=n)
    index = index.cpu().numpy().reshape(-1)
    print(H, W, index.tolist())
    assert np.array_equal(index[sel], np.arange(n))                  # every point's key sits on its own pixel
    mask, any_ = hipops.points_in_fov(cloud[:n], cams, H, W, FOV_RANGE)
    assert mask.cpu().numpy().all() and any_.cpu().tolist() == [1]
