"""Host side of the D4 augmentation (nextbestpath_amd/utility/augment.py): the heading permutation from the camera code, the group
structure, the geometry against the map oracle, the targets, and the draws.  No GPU."""
import random

import numpy as np
import pytest

from nextbestpath_amd.utility import augment
from oracle import maps as omaps

OPS = list(range(8))


def restate(a, op):
    """The index rule of the issue, written as one gather (independent of augment.transform_maps' slicing):
    out[r][c] = A[fr ? n - r : r][fc ? n - c : c], A = in^T when bit 0 is set, 0 where the source index is n."""
    a = np.asarray(a)
    n = a.shape[-1]
    R, C = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rp = n - R if op & 2 else R
    cp = n - C if op & 4 else C
    ok = (rp < n) & (cp < n)
    rp, cp = np.minimum(rp, n - 1), np.minimum(cp, n - 1)
    sr, sc = (cp, rp) if op & 1 else (rp, cp)
    return np.where(ok, a[..., sr, sc], 0).astype(a.dtype)


def _vec_op(v, op):
    """The op's 2 x 2 signed permutation on a (d_row, d_col) direction."""
    dr, dc = v
    if op & 1:
        dr, dc = dc, dr
    if op & 2:
        dr = -dr
    if op & 4:
        dc = -dc
    return np.array([dr, dc])


def _heading_dir(c):
    """(d_row, d_col) of heading c from the camera code: the look direction is the camera's z axis (third column of R);
    row ~ -(z - c_z), col ~ -(x - c_x)."""
    from nextbestpath_amd.simulator.camera import _look_rotation
    look = _look_rotation((0.0, 45.0 * c))[:, 2]
    assert abs(look[1]) < 1e-12 and abs(np.hypot(look[0], look[2]) - 1.0) < 1e-12
    return np.array([-look[2], -look[0]])


def test_heading_permutation_from_the_camera_code():
    dirs = [_heading_dir(c) for c in range(8)]
    for c in range(8):            # the docstring's (d_row, d_col) = (-cos a, -sin a)
        a = np.deg2rad(45.0 * c)
        assert np.abs(dirs[c] - np.array([-np.cos(a), -np.sin(a)])).max() < 1e-12
    for op in OPS:
        hm = augment.heading_map(op)
        assert hm.shape == (8,) and sorted(hm.tolist()) == list(range(8))
        for c in range(8):
            v = _vec_op(dirs[c], op)
            match = [h for h in range(8) if np.abs(dirs[h] - v).max() < 1e-12]
            assert match == [int(hm[c])], (op, c, match, hm)


def test_group_structure():
    S = 32
    rng = np.random.default_rng(0)
    a = rng.random((S, S)).astype(np.float32)
    a[0, :] = 0
    a[:, 0] = 0
    imgs = [augment.transform_maps(a, op) for op in OPS]
    for op in OPS:
        assert np.array_equal(imgs[op], restate(a, op))
    assert np.array_equal(imgs[0], a)
    for i in OPS:
        for j in OPS:
            assert (i == j) == np.array_equal(imgs[i], imgs[j])
    h0 = np.arange(8)
    for i in OPS:
        # the composition "i then j" is one of the eight, for the arrays and for the headings alike
        for j in OPS:
            comp = augment.transform_maps(imgs[i], j)
            ks = [k for k in OPS if np.array_equal(comp, imgs[k])]
            assert len(ks) == 1
            assert np.array_equal(augment.heading_map(j)[augment.heading_map(i)], augment.heading_map(ks[0]))
        inv = [j for j in OPS if np.array_equal(augment.transform_maps(imgs[i], j), a)]
        assert len(inv) == 1
        assert np.array_equal(augment.heading_map(inv[0])[augment.heading_map(i)], h0)
    with pytest.raises(ValueError):
        augment.heading_map(8)


def test_reflection_zeroes_index_zero_and_is_not_an_array_flip():
    a = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
    r = augment.transform_maps(a, 2)
    assert np.array_equal(r[0], np.zeros(4)) and np.array_equal(r[1], a[3]) and np.array_equal(r[3], a[1])
    assert not np.array_equal(r, a[::-1])
    c = augment.transform_maps(a, 4)
    assert np.array_equal(c[:, 0], np.zeros(4)) and np.array_equal(c[:, 1], a[:, 3])
    assert np.array_equal(a, np.arange(1, 17, dtype=np.float32).reshape(4, 4))


POSE = (12.25, 1.5, -7.5)
Y_BINS = (-1.0, 0.5, 2.0, 3.5, 5.0)


def seeded_cloud(n=20000, seed=7):
    """Offsets from the camera on a 2^-14 grid within +-45 units: camera + offset, and camera + transformed offset, are exact in
    fp32, so the two map builds see exactly mirrored offsets and only the index rule itself is under test."""
    rng = np.random.default_rng(seed)
    off = np.round(rng.uniform(-45.0, 45.0, (n, 2)) * 2.0 ** 14) / 2.0 ** 14          # (x, z) offsets
    y = rng.uniform(-2.0, 6.0, n)
    return off, y


def cloud_points(off, y, op):
    """World points of the cloud moved by `op` about the camera: bit 0 swaps the x and z offsets, bit 1 negates the z offset
    (rows ~ -(z - c_z)), bit 2 negates the x offset (cols ~ -(x - c_x)); in that order."""
    ox, oz = off[:, 0], off[:, 1]
    if op & 1:
        ox, oz = oz, ox
    if op & 2:
        oz = -oz
    if op & 4:
        ox = -ox
    p = np.stack([POSE[0] + ox, y, POSE[2] + oz], 1)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32[:, [0, 2]].astype(np.float64), p[:, [0, 2]])          # exact in fp32
    return p32


def near_tie_cells(off, op, S, window=1e-4):
    """[S,S] mask, in the frame of the maps moved by `op`, of the cells a point within `window` cells of a half-cell tie of rint
    can land in (fp32 rounding of (v + 40) * scale is not mirror-symmetric to the last bit: 3e-5 cells at most)."""
    ox, oz = off[:, 0], off[:, 1]
    if op & 1:
        ox, oz = oz, ox
    if op & 2:
        oz = -oz
    if op & 4:
        ox = -ox
    u = np.stack([(-oz + 40.0) * S / 80.0, (-ox + 40.0) * S / 80.0], 1)              # (row, col) cell coordinates, float64
    tie = (np.abs(u - np.floor(u) - 0.5) < window).any(1)
    mask = np.zeros((S, S), dtype=bool)
    for ur, uc in u[tie]:
        for r in (int(np.floor(ur)), int(np.ceil(ur))):
            for c in (int(np.floor(uc)), int(np.ceil(uc))):
                if 0 <= r < S and 0 <= c < S:
                    mask[r, c] = True
    return mask


@pytest.mark.parametrize("op", OPS[1:])
def test_geometry_against_the_map_oracle(op):
    S = 256
    off, y = seeded_cloud()
    first = omaps.accumulate_step_maps(cloud_points(off, y, 0), POSE, Y_BINS, S=S)
    second = omaps.accumulate_step_maps(cloud_points(off, y, op), POSE, Y_BINS, S=S)
    assert first[:5].sum() > 15000 and first[:4].sum() > 5000                           # the cloud is in the window and in the slabs
    moved = restate(first, op)
    assert np.array_equal(moved, augment.transform_maps(first, op))
    diff = (moved != second)[:, 1:, 1:]
    ties = near_tie_cells(off, op, S)[1:, 1:]
    assert not (diff & ~ties[None]).any(), f"op {op}: {int((diff & ~ties[None]).sum())} cells differ away from rint ties"
    n_tie = int(diff.sum())
    print(f"op {op}: {n_tie} tie cells excluded of {diff.size}")
    assert n_tie * 10000 < diff.size


def _cell(pose_a, pose_j, V):
    """Value-grid cell of pose j in pose a's frame (the map rule: i = rint((v + 40) V / 80), v = -(offset))."""
    v = np.array([-(pose_j[2] - pose_a[2]), -(pose_j[0] - pose_a[0])], dtype=np.float32)
    return omaps._cells(v, V, (-40, 40)).astype(np.int64)


@pytest.mark.parametrize("op", OPS)
def test_targets_follow_the_poses(op):
    V = 64
    rng = np.random.default_rng(3)
    a = np.array([5.0, 1.5, -2.5])
    # lattice neighbours of pose a (steps of 1.25 units = one value cell: no rint ties), the far edge v = -40 among them
    steps = np.concatenate([rng.integers(-31, 32, (40, 2)), [[32, 3], [-5, 32], [32, 32], [0, 0]]])
    pix, gains, want = [], [], []
    for k, (sx, sz) in enumerate(steps):
        j = a + np.array([1.25 * sx, 0.0, 1.25 * sz])
        r, c = _cell(a, j, V)
        h = k % 8
        pix.append((h, r, c))
        gains.append(0.25 * k)
        ox, oz = j[0] - a[0], j[2] - a[2]
        if op & 1:
            ox, oz = oz, ox
        if op & 2:
            oz = -oz
        if op & 4:
            ox = -ox
        r2, c2 = _cell(a, a + np.array([ox, 0.0, oz]), V)
        if 0 <= r2 < V and 0 <= c2 < V:
            want.append((int(augment.heading_map(op)[h]), r2, c2, 0.25 * k))
    pix, gains = np.array(pix, dtype=np.int64), np.array(gains, dtype=np.float32)
    assert (pix[:, 1:] >= 0).all() and (pix[:, 1:] < V).all() and (pix[:, 1] == 0).sum() == 2 and (pix[:, 2] == 0).sum() == 2
    pix0, gains0 = pix.copy(), gains.copy()
    p2, g2 = augment.transform_targets(pix, gains, op, V)
    assert np.array_equal(pix, pix0) and np.array_equal(gains, gains0)                # inputs are not modified
    assert p2.dtype == np.int64 and g2.dtype == np.float32 and p2.shape == (len(want), 3)
    assert [tuple(p) + (float(g),) for p, g in zip(p2.tolist(), g2)] == want          # gains travel with their targets, in order
    p2[:] = -1                                                                        # ... and the result owns its memory
    assert np.array_equal(pix, pix0)


def test_targets_on_row_zero():
    V = 16
    pix = np.array([[3, 0, 5], [1, 4, 0], [7, 2, 9]], dtype=np.int64)
    g = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    p, q = augment.transform_targets(pix, g, 2, V)            # reflect rows: the row-0 target leaves the grid
    assert p.tolist() == [[3, 12, 0], [5, 14, 9]] and q.tolist() == [2.0, 3.0]
    p, q = augment.transform_targets(pix, g, 1, V)            # transpose keeps it
    assert p.tolist() == [[7, 5, 0], [1, 0, 4], [3, 9, 2]] and q.tolist() == [1.0, 2.0, 3.0]
    p, q = augment.transform_targets(pix, g, 6, V)
    assert p.tolist() == [[3, 14, 7]] and q.tolist() == [3.0]          # a half turn: heading 7 -> 7 + 4
    p, q = augment.transform_targets(np.zeros((0, 3), np.int64), np.zeros(0, np.float32), 5, V)
    assert p.shape == (0, 3) and q.shape == (0,)


def test_augment_records_leaves_the_records_alone():
    rec = [{"target_value_map_pixel": np.array([[1, 0, 2], [2, 3, 4]], dtype=np.int64),
            "actual_coverage_gain": np.array([1.0, 2.0], dtype=np.float32), "pose_i": 20 + i, "current_model_input": None}
           for i in range(3)]
    before = [(d["target_value_map_pixel"].copy(), d["actual_coverage_gain"].copy()) for d in rec]
    out = augment.augment_records(rec, np.array([0, 2, 1], dtype=np.int32), 16)
    assert out[0] is rec[0] and out[1] is not rec[1] and out[1]["pose_i"] == 21
    assert out[1]["target_value_map_pixel"].tolist() == [[2, 13, 4]] and out[1]["actual_coverage_gain"].tolist() == [2.0]
    assert out[2]["target_value_map_pixel"].tolist() == [[1, 2, 0], [0, 4, 3]]
    for d, (p, g) in zip(rec, before):
        assert np.array_equal(d["target_value_map_pixel"], p) and np.array_equal(d["actual_coverage_gain"], g)


def test_draw_ops():
    rng = random.Random(11)
    state = rng.getstate()
    z = augment.draw_ops(rng, 50, 0.0)
    assert z.dtype == np.int32 and z.shape == (50,) and not z.any() and rng.getstate() == state
    glob = random.getstate()
    one = augment.draw_ops(rng, 4000, 1.0)
    assert one.min() >= 1 and one.max() <= 7
    counts = np.bincount(one, minlength=8)[1:]
    assert counts.min() > 4000 / 7 * 0.8 and counts.max() < 4000 / 7 * 1.2          # uniform over the seven (5 sigma is 0.19)
    assert np.array_equal(augment.draw_ops(random.Random(4), 100, 0.4), augment.draw_ops(random.Random(4), 100, 0.4))
    half = augment.draw_ops(random.Random(5), 4000, 0.5)
    assert 0.45 < (half != 0).mean() < 0.55
    assert random.getstate() == glob                                                  # the global generator is never touched
