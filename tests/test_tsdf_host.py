"""The TSDF fusion's definition (nextbestpath_amd/utility/tsdf.py), pinned without a GPU: the option's accept / refuse rules, the
volume geometry's known answers, the vectorised functions against the plain nested-loop transcription, the order-freedom of the
integer state, and what the fused cloud must be on scenes whose answer is known: a fronto-parallel plane (every point within the
quantisation step of it), a two-plane step (no false sheet at the silhouette), noisy frames (the noise averages out) and
min_weight."""
import numpy as np
import pytest

from nextbestpath_amd.utility import tsdf

f32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
H, W = 64, 114                                   # the plane scenes' frame
DIMS, VOXEL, TRUNC = (32, 32, 48), 0.25, 1.0     # ... and volume: 8 x 8 x 12 units in front of the identity camera
LO = np.array([-4.0, -4.0, 0.0], f32)


# ---------------------------------------------------------------------------------------------------------------- the option
def test_option_none_and_defaults():
    assert tsdf.option_spec(None) is None and tsdf.option_spec(False) is None
    assert tsdf.option_spec(True) == {"voxel": 0.25, "trunc": 1.0, "min_weight": 1}
    got = tsdf.option_spec({"voxel": 0.5, "trunc": np.float32(1.0), "max_depth": 30, "min_weight": np.int64(3)})
    assert got == {"voxel": 0.5, "trunc": 1.0, "min_weight": 3, "max_depth": 30.0}
    assert isinstance(got["trunc"], float) and isinstance(got["min_weight"], int) and isinstance(got["max_depth"], float)
    assert tsdf.option_spec(got) == got                               # a normalised spec is a fixed point
    assert tsdf.resolved_options(tsdf.option_spec(True), 70)["max_depth"] == 70.0
    assert tsdf.resolved_options(got, 70)["max_depth"] == 30.0


@pytest.mark.parametrize("bad", [
    1, "on", [], ("voxel", 0.25), {"voxels": 0.25}, {"voxel": 0}, {"voxel": -1.0}, {"voxel": float("nan")}, {"voxel": float("inf")},
    {"voxel": "0.25"}, {"voxel": True}, {"trunc": 0}, {"trunc": float("inf")}, {"trunc": 0.49}, {"voxel": 0.6}, {"max_depth": 0},
    {"max_depth": float("nan")}, {"max_depth": float("inf")}, {"max_depth": None}, {"min_weight": 0}, {"min_weight": 1.0},
    {"min_weight": True}, {"min_weight": -2},
])
def test_option_refusals(bad):
    with pytest.raises(ValueError):
        tsdf.option_spec(bad)


def test_trunc_of_exactly_two_voxels_is_accepted():
    assert tsdf.option_spec({"voxel": 0.5, "trunc": 1.0})["trunc"] == 1.0


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_geometry_known_answers():
    spec = tsdf.option_spec(True)
    lo, dims = tsdf.volume_geometry(([0, 0, 0], [10, 2.1, 3]), spec)
    assert lo.dtype == f32 and lo.tolist() == [-1.0, -1.0, -1.0]
    assert dims.tolist() == [48, 17, 20]                              # 12 / 0.25, ceil(4.1 / 0.25), 5 / 0.25
    lo, dims = tsdf.volume_geometry(([-3.5, 1, 2], [-3.5, 1, 2]), tsdf.option_spec({"voxel": 0.5, "trunc": 1.25}))
    assert lo.tolist() == [-4.75, -0.25, 0.75] and dims.tolist() == [5, 5, 5]
    c = tsdf.axis_centres([-1, -1, -1], 0.25, [48, 17, 20])
    assert [a.dtype for a in c] == [f32] * 3 and c[0][0] == f32(-0.875) and c[1][16] == f32(3.125) and c[2][19] == f32(3.875)
    assert tsdf.voxel_centres([-1, -1, -1], 0.25, [2, 3, 4])[(1 * 3 + 2) * 4 + 3].tolist() == [-0.625, -0.375, -0.125]
    assert tsdf.empty_volume([2, 3, 4]).shape == (2, 3, 4, 2) and tsdf.empty_volume([2, 3, 4]).dtype == np.int32
    assert float(tsdf.scale_of(1.0)) == 127.0 and tsdf.scale_of(0.3) == f32(127) / f32(0.3)


def test_geometry_refusals():
    spec = tsdf.option_spec(True)
    tsdf.volume_geometry(([0, 0, 0], [158, 158, 158]), spec)          # 640^3 = 2^27.9...
    with pytest.raises(ValueError):
        tsdf.volume_geometry(([0, 0, 0], [200, 200, 200]), spec)      # 808^3 > 2^28
    with pytest.raises(ValueError):
        tsdf.volume_geometry(([0, 0, 0], [1, -1, 1]), spec)
    with pytest.raises(ValueError):
        tsdf.volume_geometry(([0, 0, 0], [1, float("nan"), 1]), spec)


# ---------------------------------------------------------------------------------------------------------------- transcription
def rotated_camera(rng, centre, distance):
    """A camera at `distance` from `centre`, looking roughly at it, with a random roll: (R, T) with X_view = X R + T."""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    eye = np.asarray(centre, np.float64) - distance * q[:, 2]         # the centre lies `distance` down the view's z axis
    return np.concatenate([q.reshape(-1), -(eye @ q)]).astype(f32)


def small_scene(seed, n_frames=3, shape=(9, 14)):
    rng = np.random.default_rng(seed)
    lo, voxel, dims = np.array([-0.7, 0.2, 1.1], f32), 0.3, (5, 4, 6)
    centre = lo + 0.5 * voxel * np.array(dims)
    cams = [rotated_camera(rng, centre, d) for d in rng.uniform(1.5, 4.0, n_frames)]
    frames = []
    for d in rng.uniform(1.5, 4.0, n_frames):
        z = rng.uniform(d - 1.0, d + 1.0, shape).astype(f32)
        z[rng.random(shape) < 0.15] = -1.0
        z[rng.random(shape) < 0.05] = np.nan
        frames.append(z)
    return lo, voxel, dims, frames, cams


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_equals_scalar_transcription(seed):
    lo, voxel, dims, frames, cams = small_scene(seed)
    trunc, max_depth = 0.6, 4.2
    a, b = tsdf.empty_volume(dims), tsdf.empty_volume(dims)
    for z, cam in zip(frames, cams):
        tsdf.integrate(a, lo, voxel, z, cam, trunc, max_depth)
        tsdf.integrate_scalar(b, lo, voxel, z, cam, trunc, max_depth)
        assert np.array_equal(a, b)
    assert (a[..., 1] > 0).sum() > 20 and (a[..., 1] == 0).any() and (a[..., 0] < 0).any() and (a[..., 0] > 0).any()
    for mw in (1, 2):
        p, q = tsdf.extract(a, lo, voxel, mw), tsdf.extract_scalar(a, lo, voxel, mw)
        assert p.dtype == q.dtype == f32 and p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32))
        assert tsdf.stats(a, mw) == tsdf.stats_scalar(a, mw)
    assert len(tsdf.extract(a, lo, voxel, 1)) > 0


def test_permuting_and_regrouping_frames_gives_identical_volumes():
    """The state is a pair of integer sums per voxel: the frames' order and grouping cannot matter."""
    lo, voxel, dims, frames, cams = small_scene(11, n_frames=5)
    want = tsdf.empty_volume(dims)
    for z, cam in zip(frames, cams):
        tsdf.integrate(want, lo, voxel, z, cam, 0.6, 4.2)
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        got = tsdf.empty_volume(dims)
        for i in order:
            tsdf.integrate(got, lo, voxel, frames[i], cams[i], 0.6, 4.2)
        assert np.array_equal(got, want)
    parts = []
    for group in ([0, 3], [4], [1, 2]):                               # three volumes of a group each, added afterwards
        v = tsdf.empty_volume(dims)
        for i in group:
            tsdf.integrate(v, lo, voxel, frames[i], cams[i], 0.6, 4.2)
        parts.append(v)
    assert np.array_equal(parts[0] + parts[1] + parts[2], want)


# ---------------------------------------------------------------------------------------------------------------- known scenes
def fuse(frames, min_weight=1, max_depth=70.0):
    vol = tsdf.empty_volume(DIMS)
    for z in frames:
        tsdf.integrate(vol, LO, VOXEL, z, IDENTITY, TRUNC, max_depth)
    return vol, tsdf.extract(vol, LO, VOXEL, min_weight)


@pytest.mark.parametrize("n_frames", [1, 8])
def test_plane_is_recovered_within_the_quantisation_step(n_frames):
    _, pts = fuse([np.full((H, W), 8.03, f32)] * n_frames)
    assert len(pts) > 500
    err = float(np.abs(pts[:, 2].astype(np.float64) - 8.03).max())
    print(f"plane: {len(pts)} points, max |z - 8.03| = {err:.5f} (bound {TRUNC / 127:.5f})")
    assert err <= TRUNC / 127


def test_step_scene_has_no_false_sheet():
    z = np.full((H, W), 5.03, f32)
    z[:, W // 2:] = 9.03
    vol, pts = fuse([z])
    far = np.minimum(np.abs(pts[:, 2] - 5.03), np.abs(pts[:, 2] - 9.03)) > 0.3
    print(f"step scene: {int(far.sum())} of {len(pts)} points farther than 0.3 from both planes")
    assert len(pts) > 500 and not far.any()
    # the rule that does it: without the saturated-voxel exclusion the silhouette grows a sheet between the planes
    S, Wt = vol[..., 0].astype(np.int64), vol[..., 1].astype(np.int64)
    assert ((Wt > 0) & (np.abs(S) == 127 * Wt)).any()


def test_noise_averages_out():
    rng = np.random.default_rng(0)
    sigma = 0.1
    frames = [(8.03 + rng.standard_normal((H, W)) * sigma).astype(f32) for _ in range(8)]
    raw = float(np.sqrt(np.mean([np.mean((f.astype(np.float64) - 8.03) ** 2) for f in frames])))
    _, pts = fuse(frames)
    fused = float(np.sqrt(np.mean((pts[:, 2].astype(np.float64) - 8.03) ** 2)))
    print(f"noise: fused z-RMSE {fused:.4f} against the raw frames' {raw:.4f} (ratio {fused / raw:.3f}; 1 / sqrt(8) = 0.354)")
    assert len(pts) > 500 and fused < 0.5 * raw


def test_min_weight_excludes_voxels_seen_once():
    full = np.full((H, W), 8.03, f32)
    half = full.copy()
    half[:, W // 2:] = -1.0                                           # the second frame sees the left half only (x > 0)
    vol, once = fuse([full, half], min_weight=1)
    _, twice = fuse([full, half], min_weight=2)
    assert vol[..., 1].max() == 2 and 0 < len(twice) < len(once)
    assert twice[:, 0].min() > -0.2 and once[:, 0].min() < -3.0       # (a column's x falls as it rises: the left half is x > 0)
    assert len(fuse([full], min_weight=2)[1]) == 0
    assert tsdf.stats(vol, 2)["usable_voxels"] < tsdf.stats(vol, 1)["usable_voxels"] <= tsdf.stats(vol, 1)["observed_voxels"]


def test_invalid_and_far_depths_are_not_integrated():
    z = np.full((H, W), 8.03, f32)
    for bad in (-1.0, np.nan, np.inf, 70.5):
        vol, pts = fuse([np.full((H, W), bad, f32)])
        assert not vol.any() and len(pts) == 0
    vol, _ = fuse([z], max_depth=8.0)
    assert not vol.any()
    vol, _ = fuse([z], max_depth=float(f32(8.03)))
    assert vol.any()


def test_raw_row_round_trip():
    from nextbestpath_amd.utility import recon_metrics as rm
    row = rm.pack_raw([3.5, 9.25], [7, 9], 12, [4.5, 11.0], [5, 6], 20)
    raw = tsdf.pack_raw(row, 2 ** 27 + 1, 12345, 505)
    block = tsdf.summarise_raw(raw, (0.5, 1.0), 5.0, {"voxel": 0.25})
    want = rm.summarise_raw(row, (0.5, 1.0), 5.0)
    assert {k: block[k] for k in want} == want
    assert (block["observed_voxels"], block["usable_voxels"], block["frames"]) == (2 ** 27 + 1, 12345, 505)
    assert block["options"] == {"voxel": 0.25} and block["n_points"] == 12
