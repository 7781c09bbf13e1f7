"""The cameras, clouds and ground-truth images that the held-out view metrics' host and GPU tests share
(tests/test_view_metrics_host.py, tests/test_gpu_views.py), and their numpy references (utility/view_metrics.py), computed once
per process."""
import functools

import numpy as np

from nextbestpath_amd.utility import view_metrics as vm
from oracle import camera as ocam

f32 = np.float32
Z_FAR = 60.0                                  # below the deepest points (70): some lie beyond it
TAU = 1.0
SIZES = ((24, 40), (40, 24), (7, 5))
N_POINTS = (1, 255, 256, 257, 5000)           # around a block's 256 threads; 5000: more than one block


def cams12(R, T):
    return np.concatenate([np.asarray(R, f32).reshape(-1, 9), np.asarray(T, f32).reshape(-1, 3)], 1)


@functools.lru_cache(maxsize=None)
def lattice_cams(n, seed=3):
    """[n,12]: camera 0 is the identity (R = I, T = 0: view space is world space, so a test can place a point's v exactly), the
    others lattice-like poses (positions on a 3-unit grid, elevation 0 or -30, headings in steps of 45 degrees) that look at the
    region in front of camera 0."""
    rng = np.random.default_rng(seed)
    out = [np.concatenate([np.eye(3, dtype=f32).reshape(-1), np.zeros(3, f32)])]
    while len(out) < n:
        X = np.array([3.0 * rng.integers(-3, 4), 3.3, 3.0 * rng.integers(-2, 6)])
        R, T = ocam.camera_RT(X, (float(rng.choice([0.0, -30.0])), 45.0 * rng.integers(0, 8)))
        out.append(np.concatenate([R.reshape(-1), T]))
    a = np.stack(out).astype(f32)
    a.setflags(write=False)
    return a


def unproject_rc(rows, cols, z, R, T, H, W):
    """oracle/camera.py::unproject's arithmetic for arbitrary integer (row, col), also outside the image."""
    s = min(H, W)
    rows, cols, z = np.asarray(rows, f32), np.asarray(cols, f32), np.asarray(z, f32)
    ndc_x = f32(W / s) - (cols / f32(s - 1)) * f32(2)
    ndc_y = f32(H / s) - (rows / f32(s - 1)) * f32(2)
    xv, yv = (ndc_x * z) * ocam.TAN_HALF_FOV, (ndc_y * z) * ocam.TAN_HALF_FOV
    R, T = np.asarray(R, f32).reshape(3, 3), np.asarray(T, f32)
    dx, dy, dz = xv - T[0], yv - T[1], z - T[2]
    return np.stack([(dx * R[j, 0] + dy * R[j, 1]) + dz * R[j, 2] for j in range(3)], 1).astype(f32)


def half_integer_points(H, W, n_want=6):
    """Points in camera 0's (identity) view space whose cf + 0.5 is an exact integer (cf = k + 0.5 exactly: the pixel decision sits
    on its rounding boundary), found by walking v0 a few floats around the exact solution."""
    s = min(H, W)
    found = []
    for k in range(0, W - 1):
        for z in (f32(2.0), f32(3.7), f32(11.0)):
            t = z * vm.TAN_HALF_FOV
            nx = W / s - 2.0 * (k + 0.5) / (s - 1)
            v0 = f32(nx * float(t))
            cand = [v0]
            for _ in range(6):
                cand.append(np.nextafter(cand[-1], f32(np.inf)))
            lo = v0
            for _ in range(6):
                lo = np.nextafter(lo, f32(-np.inf))
                cand.append(lo)
            for c in cand:
                cf = ((f32(W / s) - f32(c) / t) * f32(0.5)) * f32(s - 1)
                if cf == f32(k + 0.5):
                    found.append([c, f32(0.1), z])
                    break
        if len(found) >= n_want:
            break
    return np.asarray(found, f32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def cloud_case(H, W, V):
    """-> (cams [V,12], cloud [5200,3]: 5000 rows to splat and a poisoned tail, colours [5200,3]).  The first 250 rows hold the
    special points (so that every prefix length of the tests but 1 meets them), the rest are pixels of the V cameras un-projected
    at depths 0.6 .. 70."""
    cams = lattice_cams(V)
    rng = np.random.default_rng(1000 * H + 10 * W + V)
    I3, T0 = np.eye(3, dtype=f32), np.zeros(3, f32)
    sp = []
    sp.append(np.array([[0.1, 0.2, -3.0], [0.0, 0.0, 0.0], [0.3, -0.1, -0.5]], f32))                  # behind camera 0, and at its centre
    zc = f32(vm.Z_CLIP)
    sp.append(np.array([[0.01, 0.01, zc], [0.01, 0.02, np.nextafter(zc, f32(1))], [0.0, 0.0, np.nextafter(zc, f32(0))]], f32))
    zf = f32(Z_FAR)
    sp.append(np.array([[0.5, 0.5, zf], [0.5, 0.4, np.nextafter(zf, f32(0))], [0.4, 0.5, np.nextafter(zf, f32(100))]], f32))
    # outside every border of camera 0 by 1 .. 5 pixels (less than, equal to and more than the radii of the tests)
    for d in (1, 2, 4, 5):
        n = 6
        z = rng.uniform(1.0, 30.0, n).astype(f32)
        sp.append(unproject_rc(rng.integers(0, H, n), np.full(n, -d), z, I3, T0, H, W))
        sp.append(unproject_rc(rng.integers(0, H, n), np.full(n, W - 1 + d), z, I3, T0, H, W))
        sp.append(unproject_rc(np.full(n, -d), rng.integers(0, W, n), z, I3, T0, H, W))
        sp.append(unproject_rc(np.full(n, H - 1 + d), rng.integers(0, W, n), z, I3, T0, H, W))
        sp.append(unproject_rc([-d, -d, H - 1 + d, H - 1 + d], [-d, W - 1 + d, -d, W - 1 + d], z[:4], I3, T0, H, W))   # the corners
    half = half_integer_points(H, W)
    assert len(half) >= 1, (H, W)
    sp.append(half)
    sp.append(np.array([[np.nan, 0, 5], [0, np.inf, 5], [0, 0, -np.inf], [np.inf, np.inf, np.inf], [0, 0, np.nan], [1e30, 1e30, 1e30],
                        [-1e38, 3e38, 1.0]], f32))
    special = np.concatenate(sp)
    bulk = []
    n_bulk = 5000 - len(special) - 40
    per = -(-n_bulk // V)
    for c in range(V):
        z = rng.uniform(0.6, 70.0, per).astype(f32)
        bulk.append(unproject_rc(rng.integers(0, H, per), rng.integers(0, W, per), z, cams[c, :9].reshape(3, 3), cams[c, 9:], H, W))
    bulk = np.concatenate(bulk)[:n_bulk]
    rng.shuffle(bulk)
    cloud = np.concatenate([special, bulk[:250 - len(special) - 20], bulk[100:120], bulk[250 - len(special) - 20:], special[:20]])
    assert len(special) < 200 and cloud.shape == (5000, 3)            # (rows 230..250 and the last 20: exact duplicates)
    tail = np.concatenate([np.full((100, 3), np.nan, f32), np.full((50, 3), 1e30, f32),
                           unproject_rc(rng.integers(0, H, 50), rng.integers(0, W, 50), np.full(50, 0.55, f32), I3, T0, H, W)])
    cloud = np.concatenate([cloud, tail]).astype(f32)                  # beyond the count: NaN, 1e30 and would-be nearest points
    rgb = rng.uniform(0, 1, cloud.shape).astype(f32)
    for a in (cloud, rgb):
        a.setflags(write=False)
    return cams, cloud, rgb


@functools.lru_cache(maxsize=None)
def keys_reference(H, W, V, radius, n):
    """view_metrics.splat of the first n rows of cloud_case(H, W, V)."""
    cams, cloud, _ = cloud_case(H, W, V)
    k = vm.splat(cloud[:n], cams, H, W, radius, Z_FAR)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def gt_case(H, W, V, radius, n):
    """Ground-truth images for keys_reference(H, W, V, radius, n): z_gt holds background, depths beyond Z_FAR, and around the
    splatted depth every boundary of the four classes (|dz| = tau exactly and one float either side, both signs); rgb_gt random."""
    rng = np.random.default_rng(7 + n + radius)
    z_c, _, _ = vm.resolve(keys_reference(H, W, V, radius, n))
    base = np.where(z_c > 0, z_c, rng.uniform(1, 50, z_c.shape).astype(f32)).astype(f32)
    tau = f32(TAU)
    choice = rng.integers(0, 12, z_c.shape)
    z_gt = base + rng.uniform(-3, 3, z_c.shape).astype(f32)
    z_gt = np.where(choice == 0, f32(-1), z_gt)
    z_gt = np.where(choice == 1, f32(Z_FAR) + f32(1), z_gt)
    z_gt = np.where(choice == 2, base, z_gt)
    for code, delta in ((3, tau), (4, -tau)):
        z_gt = np.where(choice == code, base - delta, z_gt)           # z_c - z_gt = +-tau up to the rounding of the subtraction
    z_gt = np.where(choice == 5, np.nextafter(base - tau, f32(-1e9)), z_gt)
    z_gt = np.where(choice == 6, np.nextafter(base - tau, f32(1e9)), z_gt)
    z_gt = np.where(choice == 7, np.nextafter(base + tau, f32(-1e9)), z_gt)
    z_gt = np.where(choice == 8, np.nextafter(base + tau, f32(1e9)), z_gt)
    z_gt = z_gt.astype(f32)
    rgb_gt = rng.uniform(0, 1, z_c.shape + (3,)).astype(f32)
    z_gt.setflags(write=False)
    rgb_gt.setflags(write=False)
    return z_gt, rgb_gt


def assert_summaries_equal(got, want, rel=1e-10):
    """Two summarise_raw dicts: the counts and the ratios of counts equal, the float64 sums' ratios within `rel` (sums of
    non-negative float64 terms added in two orders)."""
    assert set(got) == set(want)
    for key in ("n_views", "n_gt", "n_c", "n_hit", "view_completeness", "hole", "leak", "floater"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["per_view"]["view_completeness"] == want["per_view"]["view_completeness"]

    def close(a, b, what):
        assert (a is None) == (b is None), (what, a, b)
        if a is not None:
            assert abs(a - b) <= rel * max(abs(b), 1.0), (what, a, b)

    for key in ("depth_mae", "depth_rmse", "psnr"):
        close(got[key], want[key], key)
    assert len(got["per_view"]["psnr"]) == len(want["per_view"]["psnr"])
    for a, b in zip(got["per_view"]["psnr"], want["per_view"]["psnr"]):
        close(a, b, "per_view psnr")
    if "options" in want:
        assert got["options"] == want["options"]
