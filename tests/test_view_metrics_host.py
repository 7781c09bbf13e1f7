"""Host: the numpy definition of the held-out view metrics (utility/view_metrics.py) -- projection round trip, splat rules,
classes at their boundaries, summaries without denominators, the option and the choice of evaluation poses."""
import json

import numpy as np
import pytest

import view_cases as vc
from nextbestpath_amd.utility import view_metrics as vm
from oracle import camera as ocam

f32 = np.float32
I12 = np.concatenate([np.eye(3, dtype=f32).reshape(-1), np.zeros(3, f32)])[None]


def _up(x):
    return np.nextafter(f32(x), f32(np.inf))


def _down(x):
    return np.nextafter(f32(x), f32(-np.inf))


@pytest.mark.parametrize("H,W", [(12, 20), (24, 40), (40, 24), (64, 114), (256, 456)])
def test_every_unprojected_pixel_projects_onto_itself(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    cams = vc.lattice_cams(6, seed=11)
    rows, cols = np.divmod(np.arange(H * W), W)
    worst_c, worst_z = 0.0, 0.0
    for c in range(6):
        R, T = cams[c, :9].reshape(3, 3), cams[c, 9:]
        depth = rng.uniform(0.6, 70.0, (H, W)).astype(f32)
        pts = ocam.unproject(depth, R, T)
        ok, row, col, z = vm.project(pts, R, T, H, W, z_far=np.inf)
        assert ok.all()
        assert np.array_equal(row, rows.astype(f32)) and np.array_equal(col, cols.astype(f32))
        # how far from the rounding boundary, and the depth that comes back (float64 restatement of cf)
        s = min(H, W)
        v = pts.astype(np.float64) @ R.astype(np.float64) + T.astype(np.float64)
        cf = (W / s - v[:, 0] / (v[:, 2] * float(vm.TAN_HALF_FOV))) * 0.5 * (s - 1)
        worst_c = max(worst_c, float(np.abs(cf - cols).max()))
        worst_z = max(worst_z, float(np.abs(z - depth.reshape(-1)).max()))
    print(H, W, worst_c, worst_z)
    assert worst_c < 0.01 and worst_z < 1e-4


def test_nearer_point_wins_and_equal_depth_goes_to_the_lower_index():
    H, W = 7, 5
    p = vc.unproject_rc([3, 3, 3, 3], [2, 2, 2, 2], [5.0, 4.0, 4.0, 6.0], np.eye(3), np.zeros(3), H, W)
    keys = vm.splat(p, I12, H, W, radius=0)
    z, idx, _ = vm.resolve(keys)
    assert np.count_nonzero(keys != vm.EMPTY) == 1 and idx[0, 3, 2] == 1 and z[0, 3, 2] == f32(4.0)
    assert int(keys[0, 3, 2]) == (int(np.array(4.0, f32).view(np.uint32)) << 32) | 1
    # the lower index wins wherever it stands in the array
    keys = vm.splat(p[::-1], I12, H, W, radius=0)
    assert vm.resolve(keys)[1][0, 3, 2] == 1 and vm.resolve(keys)[0][0, 3, 2] == f32(4.0)
    rgb = np.arange(12, dtype=f32).reshape(4, 3)
    assert np.array_equal(vm.resolve(keys, rgb)[2][0, 3, 2], rgb[1]) and np.all(vm.resolve(keys, rgb)[2][0, 0, 0] == 0)
    assert vm.resolve(keys)[0][0, 0, 0] == -1 and vm.resolve(keys)[1][0, 0, 0] == -1


@pytest.mark.parametrize("H,W", [(7, 5), (5, 7)])
@pytest.mark.parametrize("radius", [0, 1, 2, 4])
def test_footprints_clip_at_all_four_borders(H, W, radius):
    I3, T0 = np.eye(3), np.zeros(3)
    for (row, col) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (-1, 2), (2, -1), (H, 2), (2, W),
                       (-radius, -radius), (H - 1 + radius, W - 1 + radius), (-radius - 1, 2), (2, W + radius)):
        p = vc.unproject_rc([row], [col], [3.0], I3, T0, H, W)
        ok, r, c, _ = vm.project(p, I3, T0, H, W)
        assert ok[0] and (int(r[0]), int(c[0])) == (row, col)
        filled = vm.splat(p, I12, H, W, radius)[0] != vm.EMPTY
        want = np.zeros((H, W), bool)
        want[max(row - radius, 0):max(min(row + radius, H - 1) + 1, 0), max(col - radius, 0):max(min(col + radius, W - 1) + 1, 0)] = True
        assert np.array_equal(filled, want), (row, col)


def test_depth_limits_and_non_finite_points():
    H, W = 7, 5
    zc, zf = f32(vm.Z_CLIP), f32(30.0)
    z = np.array([zc, _up(zc), _down(zc), zf, _down(zf), _up(zf), -2.0], f32)
    p = np.stack([np.zeros(7, f32), np.zeros(7, f32), z], 1)
    ok = vm.project(p, np.eye(3), np.zeros(3), H, W, z_far=zf)[0]
    assert ok.tolist() == [False, True, False, False, True, False, False]
    bad = np.array([[np.nan, 0, 5], [0, np.inf, 5], [0, 0, np.inf], [0, 0, np.nan], [-np.inf, 0, 5], [3e38, 3e38, 0.6]], f32)
    keys = vm.splat(bad, I12, H, W, radius=4)
    assert np.all(keys == vm.EMPTY)
    assert not vm.project(bad[:5], np.eye(3), np.zeros(3), H, W)[0].any()
    with pytest.raises(ValueError):
        vm.splat(p, I12, H, W, radius=5)
    with pytest.raises(ValueError):
        vm.splat(p, I12, H, W, radius=1, first_index=vm.MAX_POINTS - 7)


@pytest.mark.parametrize("H,W", vc.SIZES)
def test_two_parts_equal_the_whole(H, W):
    cams, cloud, _ = vc.cloud_case(H, W, 9)
    for radius in (0, 1, 4):
        whole = vc.keys_reference(H, W, 9, radius, 5000)
        part = vm.splat(cloud[:2000], cams, H, W, radius, vc.Z_FAR)
        part = vm.splat(cloud[2000:5000], cams, H, W, radius, vc.Z_FAR, keys=part, first_index=2000)
        assert np.array_equal(part, whole)
        assert np.count_nonzero(whole != vm.EMPTY) > 0
    # the shared case holds what it promises: points in the rim outside camera 0's image, and on a pixel's rounding boundary
    ok, row, col, _ = vm.project(cloud[:5000], cams[0, :9], cams[0, 9:], H, W, z_far=vc.Z_FAR)
    assert (ok & (col < 0) & (col >= -4)).any() and (ok & (col > W - 1) & (col <= W + 3)).any()
    assert (ok & (row < 0) & (row >= -4)).any() and (ok & (row > H - 1) & (row <= H + 3)).any()
    assert len(vc.half_integer_points(H, W)) >= 1


def test_classes_at_the_tolerance_and_one_float_either_side():
    tau, zg = f32(1.0), f32(4.0)
    z_c = np.array([5.0, _down(5.0), _up(5.0), 3.0, _up(3.0), _down(3.0), -1.0, 5.0, -1.0, 4.0, 4.0], f32)
    z_gt = np.array([zg] * 7 + [-1.0, -1.0, 100.0, _down(60.0)], f32)
    cl = vm.classify(z_c, z_gt, tau, 60.0)
    #           dz=+tau  just below  just above  dz=-tau  above   below   empty  c no gt  nothing  gt>=zfar  gt just inside
    assert cl["hit"].tolist() == [True, True, False, True, True, False, False, False, False, False, False]
    assert cl["leak"].tolist() == [False, False, True, False, False, False, False, False, False, False, False]
    assert cl["floater"].tolist() == [False, False, False, False, False, True, False, True, False, True, True]
    assert cl["hole"].tolist() == [False, False, False, False, False, False, True, False, False, False, False]
    assert cl["gt"].tolist() == [True] * 7 + [False, False, False, True]
    # every gt pixel is in exactly one of hit / hole / leak / floater; a pixel without gt is a floater iff it is filled
    one = cl["hit"].astype(int) + cl["hole"] + cl["leak"] + (cl["floater"] & cl["gt"])
    assert np.all(one[cl["gt"]] == 1)
    counts, sums = vm.raw_stats(z_c[None, None], None, z_gt[None, None], None, tau, 60.0)
    assert counts.tolist() == [[8, 9, 4, 1, 1, 4]] and counts.dtype == np.int64 and sums.dtype == np.float64
    d = np.array([1.0, float(_down(5.0)) - 4.0, -1.0, float(_up(3.0)) - 4.0])
    assert sums[0, 0] == np.abs(d).sum() and sums[0, 1] == (d * d).sum() and sums[0, 2] == 0.0


def test_summaries_have_no_nan_whatever_is_missing():
    z = np.zeros(vm.RAW_WIDTH)
    full = np.array([100, 90, 60, 20, 5, 25, 12.0, 6.0, 0.9])
    cases = {"nothing": [z], "no_views": np.zeros((0, vm.RAW_WIDTH)), "gt_only": [[50, 0, 0, 50, 0, 0, 0, 0, 0]],
             "cloud_only": [[0, 40, 0, 0, 0, 40, 0, 0, 0]], "no_hits": [[50, 40, 0, 10, 20, 40, 0, 0, 0]],
             "no_colours": [[100, 90, 60, 20, 5, 25, 12.0, 6.0, 0.0]], "full": [full, z, full]}
    for name, raw in cases.items():
        out = vm.summarise_raw(np.asarray(raw, np.float64).reshape(-1, vm.RAW_WIDTH), {"views": 3})
        json.dumps(out, allow_nan=False)
        assert out["options"] == {"views": 3}
        if name in ("nothing", "no_views", "cloud_only"):
            assert out["view_completeness"] is None and out["hole"] is None and out["leak"] is None
        if name in ("nothing", "no_views", "gt_only"):
            assert out["floater"] is None
        if name != "full":
            assert out["psnr"] is None
        if name in ("nothing", "no_views", "gt_only", "cloud_only", "no_hits"):
            assert out["depth_mae"] is None and out["depth_rmse"] is None
    out = vm.summarise_raw(np.asarray(cases["full"]))
    assert out["n_views"] == 3 and out["n_gt"] == 200 and out["view_completeness"] == 0.6 and out["hole"] == 0.2 and out["leak"] == 0.05
    assert out["floater"] == 50 / 180 and out["depth_mae"] == 0.2 and out["depth_rmse"] == np.sqrt(0.1)
    assert abs(out["psnr"] - 10 * np.log10(1 / (1.8 / 360))) < 1e-12
    assert out["per_view"]["view_completeness"] == [0.6, None, 0.6] and out["per_view"]["psnr"][1] is None
    assert "options" not in out
    assert np.array_equal(vm.pack_raw(np.array([[1, 2, 3, 4, 5, 6]]), np.array([[0.5, 0.25, 0.125]])), [[1, 2, 3, 4, 5, 6, 0.5, 0.25, 0.125]])
    with pytest.raises(ValueError):
        vm.summarise_raw(np.zeros((2, 8)))


def test_option_spec_accepts_and_refuses():
    assert vm.option_spec(None) is None and vm.option_spec(False) is None
    assert vm.option_spec(True) == {"views": 16, "seed": 0, "radius": 1, "depth_tolerance": 1.0} == vm.option_spec({})
    got = vm.option_spec({"views": 4, "seed": 3, "radius": 0, "depth_tolerance": 0.5, "height": 24, "width": 40, "z_far": 30})
    assert got == {"views": 4, "seed": 3, "radius": 0, "depth_tolerance": 0.5, "height": 24, "width": 40, "z_far": 30.0}
    assert vm.option_spec(got) == got                                         # a normalised spec passes unchanged
    assert vm.resolved_options(vm.option_spec(True), 256, 456, 50) == {"views": 16, "seed": 0, "radius": 1, "depth_tolerance": 1.0,
                                                                      "height": 256, "width": 456, "z_far": 50.0}
    assert vm.resolved_options(got, 256, 456, 50) == got
    json.dumps(got, allow_nan=False)
    for bad in (1, "on", [1], {"view": 4}, {"views": 0}, {"views": 2.5}, {"views": True}, {"radius": 5}, {"radius": -1}, {"radius": 1.0},
                {"seed": -1}, {"depth_tolerance": -0.1}, {"depth_tolerance": float("nan")}, {"depth_tolerance": "1"}, {"height": 1},
                {"width": 0}, {"z_far": 0.5}, {"z_far": float("inf")}, {"thresholds": [1.0]}):
        with pytest.raises(ValueError):
            vm.option_spec(bad)


def test_choose_views_on_a_cut_lattice():
    """3 x 3 lattice, node = 3 i + k, edges in the planner's +x, -x, +z, -z order; the mesh cuts every edge into column k = 2 except
    none: nodes 2, 5, 8 are reachable only from each other."""
    nodes = [(i, k) for i in range(3) for k in range(3)]
    index = {t: n for n, t in enumerate(nodes)}
    edges = []
    for n, (i, k) in enumerate(nodes):
        for nb in ((i + 1, k), (i - 1, k), (i, k + 1), (i, k - 1)):
            if nb in index:
                edges.append((n, index[nb]))
    nbrs = [[] for _ in nodes]
    for q, (a, b) in enumerate(edges):
        nbrs[a].append((b, q))
    hit = np.array([(nodes[a][1] == 2) != (nodes[b][1] == 2) for a, b in edges])
    everything = vm.choose_views(nbrs, hit, 0, 1000, 0)
    assert everything == [(n, h) for n in (0, 1, 3, 4, 6, 7) for h in range(8)]       # node-then-heading order: the whole pool
    assert vm.choose_views(nbrs, hit, 8, 1000, 0) == [(n, h) for n in (2, 5, 8) for h in range(8)]
    assert vm.choose_views(nbrs, hit, 4, 48, 5) == everything                         # exactly the pool's size: the pool
    a, b = vm.choose_views(nbrs, hit, 0, 10, 5), vm.choose_views(nbrs, hit, 0, 10, 5)
    assert a == b and len(a) == 10 and len(set(a)) == 10 and set(a) <= set(everything)
    assert vm.choose_views(nbrs, hit, 7, 10, 5) == a                                  # another start in the same component
    assert vm.choose_views(nbrs, hit, 0, 10, 6) != a
    assert {n for n, _ in vm.choose_views(nbrs, hit, 0, 40, 1)}.isdisjoint({2, 5, 8})
    assert vm.choose_views(nbrs, np.ones(len(edges), bool), 4, 16, 0) == [(4, h) for h in range(8)]    # walled in: the start alone
    assert vm.choose_views(nbrs, np.zeros(len(edges), np.int32), 4, 1000, 0) == [(n, h) for n in range(9) for h in range(8)]


def test_reference_composes_the_steps():
    H, W = 24, 40
    cams, cloud, rgb = vc.cloud_case(H, W, 8)
    z_gt, rgb_gt = vc.gt_case(H, W, 8, 1, 5000)
    rows = vm.reference(cloud[:5000], rgb[:5000], cams, z_gt, rgb_gt, 1, vc.TAU, vc.Z_FAR, raw=True)
    assert rows.shape == (8, vm.RAW_WIDTH)
    z_c, idx, rgb_c = vm.resolve(vc.keys_reference(H, W, 8, 1, 5000), rgb)
    assert idx.max() < 5000
    counts, sums = vm.raw_stats(z_c, rgb_c, z_gt, rgb_gt, vc.TAU, vc.Z_FAR)
    assert np.array_equal(rows, vm.pack_raw(counts, sums))
    assert counts[:, 2:].sum(0).min() > 0 and sums.min() > 0                          # every class occurs
    out = vm.reference(cloud[:5000], rgb[:5000], cams, z_gt, rgb_gt, 1, vc.TAU, vc.Z_FAR)
    assert out == vm.summarise_raw(rows) and 0 < out["view_completeness"] < 1 and out["psnr"] > 0
    # without colours: the depth half only
    nocol = vm.reference(cloud[:5000], None, cams, z_gt, rgb_gt, 1, vc.TAU, vc.Z_FAR)
    assert nocol["psnr"] is None and nocol["depth_mae"] == out["depth_mae"] and nocol["n_hit"] == out["n_hit"]
