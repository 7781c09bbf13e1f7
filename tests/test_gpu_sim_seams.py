"""GPU: the un-projection and the mesh ray queries of csrc/nbp_sim.hip at their seams, against oracle/camera.py and
oracle/mesh_rays.py (bit-exact / exact, as test_gpu_sim_planner.py holds them at ordinary sizes) and, for the ray test, against the
float64 segment test of tests/raster_reference.py."""
import numpy as np
import pytest
import torch

import raster_reference as rr
from nextbestpath_amd import _lib
from nextbestpath_amd.utility import hipops as ho
from oracle import camera as ocam
from oracle import mesh_rays

pytestmark = pytest.mark.gpu
D = "cuda"
POSES = [([1.0, 3.3, -2.0], [0.0, 45.0]), ([4.0, 3.3, -2.0], [30.0, 90.0]), ([4.0, 3.3, 1.0], [-30.0, 200.0])]
GUARD = -7.0


# ------------------------------------------------------------------------------------------------------------- un-projection
def _unproject(depth, g, seed, cap=None, count0=0, misalign=False):
    """-> (cloud incl. 8 guard rows, count, counts [F,2], oracle points per frame, oracle valid counts)."""
    F_, H, W = depth.shape
    RT = [ocam.camera_RT(x, v) for x, v in POSES[:F_]]
    cams = ho.cams12(np.stack([r for r, _ in RT]), np.stack([t for _, t in RT]))
    if misalign:                                                       # a view one float into its buffer: not 16-byte aligned
        buf = torch.zeros(depth.size + 1, device=D)
        buf[1:] = torch.from_numpy(depth.reshape(-1)).to(D)
        d = buf[1:].view(F_, H, W)
    else:
        d = torch.from_numpy(depth).to(D)
    assert ho.unproject_files(d, None) == (not misalign and (H * W) % 4 == 0)          # which path the launcher takes
    want, nvs = [], []
    for f in range(F_):
        pts, nv = ocam.partial_point_cloud(depth[f], None, RT[f][0], RT[f][1], g, 70.0, seed=seed, frame_index=f)
        want.append(pts); nvs.append(nv)
    if cap is None:
        cap = count0 + sum(len(w) for w in want) + 5
    cloud = torch.full((cap + 8, 3), GUARD, device=D)
    cnt = torch.tensor([count0], dtype=torch.int64, device=D)
    counts = ho.unproject_append(d, None, cams, cloud[:cap], cnt, g, 70.0, seed=seed).clone()
    torch.cuda.synchronize()
    return cloud.cpu().numpy(), int(cnt.item()), counts.cpu().numpy(), want, nvs


def _check(depth, g, seed, cap=None, count0=0, misalign=False):
    cloud, count, counts, want, nvs = _unproject(depth, g, seed, cap, count0, misalign)
    assert counts[:, 0].tolist() == nvs and counts[:, 1].tolist() == [len(w) for w in want]
    allp = np.concatenate(want, 0)
    cap = len(cloud) - 8
    n = min(len(allp), cap - count0)
    assert count == count0 + n
    assert np.array_equal(cloud[count0:count0 + n].view(np.int32), allp[:n].view(np.int32))       # bit-exact fp32
    assert (cloud[:count0] == GUARD).all() and (cloud[count0 + n:] == GUARD).all()                 # nothing else is written
    return cloud[count0:count0 + n]


def _depth(F_, H, W, seed, p_invalid=0.25):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.6, 120, (F_, H, W)).astype(np.float32)                # (beyond fov_range = 70: invalid too)
    d[rng.random((F_, H, W)) < p_invalid] = -1
    return d


@pytest.mark.parametrize("H,W", [(32, 57), (64, 64), (4, 2049)])
def test_unproject_generic_path_equals_fast_path(hip, H, W):
    """The three generic kernels (COMPACT_CHUNK = 2048 pixels per workgroup, a barrier per 256) and the fast ones (FAST_CHUNK = 4096,
    ranks by ballot) must build the same cloud for the same seed; a depth view that is not 16-byte aligned selects the generic ones."""
    d = _depth(3, H, W, 3)
    fast = _check(d, 0.3, 11, count0=5)
    generic = _check(d, 0.3, 11, count0=5, misalign=True)
    assert np.array_equal(fast.view(np.int32), generic.view(np.int32)) and len(fast) > 100


def test_unproject_generic_path_odd_pixel_count(hip):
    """H W = 31 x 57 = 1767 is no multiple of 4: the generic path, one partial chunk."""
    assert len(_check(_depth(3, 31, 57, 4), 0.3, 12)) > 100
    assert len(_check(_depth(2, 37, 111, 5), 1.0, 13)) > 1000          # 4107 pixels: two full chunks of 2048 and 11 pixels


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("H,W", [(64, 64), (64, 128), (4, 2049)])
@pytest.mark.parametrize("pattern", ["last_quad", "none", "all", "random"])
def test_unproject_chunk_seams(hip, H, W, pattern, misalign):
    """H W = 4096, 8192 (exactly one and two fast chunks, two and four generic ones) and 8196 (one quad into a third fast chunk, four
    pixels into a fifth generic one), with every pixel kept (gathering factor 1), so every list slot is read."""
    F_, HW = 2, H * W
    d = _depth(F_, H, W, 6, p_invalid=0.0 if pattern == "all" else 0.4)
    d = np.minimum(d, np.float32(60.0))
    if pattern == "last_quad":
        d.reshape(F_, HW)[:, :HW - 4] = -1
        d.reshape(F_, HW)[:, HW - 4:] = np.float32([3.0, 4.5, 6.0, 7.5])
    if pattern == "none":
        d[:] = -1
        d[1].reshape(-1)[::3] = 80.0                                   # beyond fov_range: not valid either
    got = _check(d, 1.0, 21, misalign=misalign)
    assert len(got) == {"last_quad": 8, "none": 0, "all": 2 * HW}.get(pattern, len(got))


@pytest.mark.parametrize("misalign", [False, True])
def test_unproject_gathering_factor_edges(hip, misalign):
    d = _depth(3, 16, 24, 7)
    assert len(_check(d, 0.0, 31, misalign=misalign)) == 0
    n_all = len(_check(d, 1.0, 31, misalign=misalign))
    assert n_all == int(((d > -1) & (d < 70)).sum())
    few = np.full((3, 16, 24), -1, np.float32)
    few[:, 5, 3:12] = 9.0                                              # 9 valid pixels a frame: int(9 x 0.1) = 0 kept
    assert len(_check(few, 0.1, 31, misalign=misalign)) == 0
    cloud = torch.zeros(64, 3, device=D)
    cnt = torch.zeros(1, dtype=torch.int64, device=D)
    for g in (1.5, -0.1, float("nan")):
        with pytest.raises(_lib.NbpHipError, match="NBP_E_ARG"):
            ho.unproject_append(torch.from_numpy(d).to(D), None, np.zeros((3, 12), np.float32), cloud, cnt, g, 70.0, seed=1)


@pytest.mark.parametrize("misalign", [False, True])
def test_unproject_capacity_ends_inside_the_second_frame(hip, misalign):
    d = _depth(3, 32, 40, 8)
    _, _, counts, want, _ = _unproject(d, 0.5, 41, misalign=misalign)
    k0, k1, k2 = (len(w) for w in want)
    assert min(k0, k1, k2) > 50
    got = _check(d, 0.5, 41, cap=9 + k0 + k1 // 2, count0=9, misalign=misalign)
    assert len(got) == k0 + k1 // 2


# --------------------------------------------------------------------------------------------------------------- ray queries
def _soup_mesh(n_faces, seed):
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-4, 4, (n_faces, 1, 3)) + rng.normal(0, 1.5, (n_faces, 3, 3))
    return rr.unshared(tri)


def _rays_vs_oracle(verts, faces, p0, p1):
    vd, fd = torch.from_numpy(verts).to(D), torch.from_numpy(faces).to(D)
    segs = np.ascontiguousarray(np.concatenate([p0, p1], 1).astype(np.float32))
    got = ho.segments_hit_mesh(vd, fd, torch.from_numpy(segs).to(D)).cpu().numpy().astype(bool)
    want = np.array([mesh_rays.segment_hits_mesh(a, b, verts, faces) for a, b in zip(segs[:, :3], segs[:, 3:])])
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    cnt = ho.axis_ray_counts(vd, fd, torch.from_numpy(segs[:, :3].copy()).to(D)).cpu().numpy()
    assert np.array_equal(cnt, np.array([mesh_rays.axis_ray_counts(p, verts, faces) for p in segs[:, :3]]))
    return got, cnt


@pytest.mark.parametrize("n_faces", [1, 255, 256, 257])
def test_ray_queries_face_count_at_the_block_size(hip, n_faces):
    """One 256-thread workgroup per 256 faces: the last thread of a full one, a lone thread in a second one, one face."""
    verts, faces = _soup_mesh(n_faces, n_faces)
    rng = np.random.default_rng(50)
    p0 = rng.uniform(-5, 5, (48, 3))
    p1 = p0 + rng.normal(0, 4, (48, 3))
    if n_faces in (1, 257):                                            # aim half of them at the LAST face: only its thread can answer
        c = verts[faces[-1]].mean(0)
        p0[:24] = c + rng.normal(0, 0.05, (24, 3)) - [0, 0, 3.0]
        p1[:24] = p0[:24] + [0, 0, 6.0]
    got, cnt = _rays_vs_oracle(verts, faces, p0, p1)
    assert got.any() and cnt.max() > 0


def test_ray_queries_exact_ends_and_shared_edge(hip):
    """t == length (the segment ends ON the face) and t == 0 (it starts on it) are no hits; a ray through the edge two faces share
    (u + v == 1 in one, v == 0 in the other) is one.  Dyadic coordinates: every product is exact, so the cases are what they say."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    p0 = np.array([[0.25, 0.25, -1], [0.25, 0.25, 0], [0.5, 0.5, -1], [0.25, 0.25, -1], [0.25, 0.25, -2], [0.5, 0.5, -1], [0.75, 0.75, 1]],
                  np.float64)
    p1 = np.array([[0.25, 0.25, 0], [0.25, 0.25, 1], [0.5, 0.5, 1], [0.25, 0.25, 0.5], [0.25, 0.25, -1], [0.5, 0.5, 0], [0.75, 0.75, -1]],
                  np.float64)
    got, cnt = _rays_vs_oracle(verts, faces, p0, p1)
    assert got.tolist() == [False, False, True, True, False, False, True]
    assert cnt[2].tolist() == [0, 0, 2] and cnt[1].tolist() == [0, 0, 0]                  # the shared edge counts for both faces


def test_ray_queries_segment_count_limit(hip):
    """blockIdx.y carries the segment: 65535 is the most a grid takes, 65536 is refused before anything is launched."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    two = np.array([[0.25, 0.25, -1, 0.25, 0.25, 1], [2, 2, -1, 2, 2, 1]], np.float32)
    want = [mesh_rays.segment_hits_mesh(s[:3], s[3:], verts, faces) for s in two]
    assert want == [True, False]
    vd, fd = torch.from_numpy(verts).to(D), torch.from_numpy(faces).to(D)
    segs = torch.from_numpy(np.tile(two, (32768, 1))).to(D)                                # 65536 rows
    hit = ho.segments_hit_mesh(vd, fd, segs[:65535].contiguous()).cpu().numpy()
    assert hit.shape == (65535,) and hit[0::2].all() and not hit[1::2].any()
    cnt = ho.axis_ray_counts(vd, fd, segs[:65535, :3].contiguous()).cpu().numpy()
    assert (cnt[0::2] == [0, 0, 1]).all() and (cnt[1::2] == 0).all()
    with pytest.raises(_lib.NbpHipError, match="NBP_E_ARG"):
        ho.segments_hit_mesh(vd, fd, segs)
    with pytest.raises(_lib.NbpHipError, match="NBP_E_ARG"):
        ho.axis_ray_counts(vd, fd, segs[:, :3].contiguous())
    torch.cuda.synchronize()


def test_segments_vs_float64(hip):
    """256 random segments through a maze: the fp32 kernel may differ from the float64 test only where that test is unsure (a hit
    within 1e-4 of an edge or of a segment end), and on at most 1 % of the segments."""
    from nextbestpath_amd.simulator.mesh import make_maze_mesh
    verts, faces = make_maze_mesh(seed=4, cells=12, size=60.0, height=30.0)
    rng = np.random.default_rng(60)
    p0 = rng.uniform(-28, 28, (256, 3)).astype(np.float32); p0[:, 1] = rng.uniform(1, 20, 256)
    p1 = p0 + rng.normal(0, 4, (256, 3)).astype(np.float32)
    got, _ = _rays_vs_oracle(verts, faces, p0, p1)
    hit64, unsure = rr.segments_hit64(p0, p1, verts, faces)
    differ = got != hit64
    assert not (differ & ~unsure).any(), np.nonzero(differ & ~unsure)[0]
    assert differ.sum() <= 0.01 * len(got), int(differ.sum())
    assert 20 < got.sum() < 236
