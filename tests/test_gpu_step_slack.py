"""GPU: the step kernels that were rebuilt to ride beside two resident convolution workgroups (<= 32 VGPRs, <= 16 KB of LDS, 256
threads) compute what they computed, bit for bit.  Exact equality throughout.

  * rasteriser (raster_block_body): the block's hit list goes through LDS in pieces of HITS = 320 entries (1024 before), the wave's
    tile sits in scalar registers and ballot ranks come from mbcnt.  One 64 x 72 frame (nine tiles across: an odd tile count and a
    half-empty 2 x 2 block), more than 2 x HITS small triangles inside one 64 x 64-pixel coarse tile (the piece loop wraps three times), a duplicated
    face (an equal-depth tie: the lowest face id wins), a face that crosses the near plane; single form and group form, against
    oracle/raster.py.
  * coverage (coverage_mark_body): stamps four at a time, positions one at a time.  GT columns of every run length 0 .. 2 x 4 + 1,
    clouds below and above the sample size k; single form and group form, against the brute-force count over the same perm_index
    subset (oracle/planner.py::coverage).
  * un-projection (unproject_append_body<COLOUR>): the depth-only instantiation against the colour instantiation on the same
    frames, plain call, filing call in step and out of step, group form."""
import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import hipops as ho
from nextbestpath_amd.utility import utils as hu
from oracle import camera as ocam
from oracle import planner as opl
from oracle import raster as oraster

pytestmark = pytest.mark.gpu
D = "cuda"
H, W = 64, 72
HITS = 320              # csrc/nbp_sim.hip
UNROLL = 4              # csrc/nbp_planner.hip: coverage_mark_kernel<4, 4>


class _Owner:
    """Stands in for the rollout object that owns an item's scratch (hipops._item_ws)."""


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _cams(poses):
    RT = [ocam.camera_RT(x, v) for x, v in poses]
    return RT, ho.cams12(np.stack([r for r, _ in RT]), np.stack([t for _, t in RT]), D)


# ------------------------------------------------------------------ rasteriser
POSES_A = [([0.0, 1.0, 0.0], [0.0, 0.0]), ([0.3, 1.0, -0.5], [4.0, 8.0]), ([-0.4, 1.2, 0.2], [-5.0, 352.0])]
POSES_B = [([0.5, -1.0, 2.0], [10.0, 20.0]), ([-2.0, 1.0, 0.0], [-35.0, 130.0]), ([2.5, 2.0, -1.5], [50.0, 220.0])]
N_DENSE = 1204          # > 2 x HITS: the coarse tile's list goes through LDS in four pieces
TIE_LO, TIE_HI = 7, N_DENSE + 1          # the duplicated face: one copy among the first entries, one behind the dense ones


def _view_to_world(view, R, T):
    return ((np.asarray(view, np.float64).reshape(-1, 3) - np.asarray(T, np.float64)) @ np.asarray(R, np.float64).T).astype(np.float32)


def _mesh_a():
    """In the view of POSES_A[0]: N_DENSE small triangles whose centres lie in image columns 4 .. 56 (one coarse tile), a large face
    at z = 2.6 in front of a part of them, listed twice (ids TIE_LO and TIE_HI), and a face from z = 4 to behind the camera."""
    R, T = ocam.camera_RT(*POSES_A[0])
    rng = np.random.default_rng(77)
    s, t = min(H, W), float(ocam.TAN_HALF_FOV)
    z = rng.uniform(3.0, 10.0, N_DENSE)
    ndc_x = rng.uniform((W - 2 * 56 - 1) / s, (W - 2 * 4 - 1) / s, N_DENSE)
    ndc_y = rng.uniform(-0.8 * H / s, 0.8 * H / s, N_DENSE)
    centre = np.stack([ndc_x * z * t, ndc_y * z * t, z], 1)
    dense = centre[:, None, :] + rng.normal(0, 0.06, (N_DENSE, 3, 3))
    x_at = lambda col, zz: (W - 2 * col - 1) / s * zz * t          # noqa: E731
    y_at = lambda row, zz: (H - 2 * row - 1) / s * zz * t          # noqa: E731
    tie = np.array([[x_at(10, 2.6), y_at(8, 2.6), 2.6], [x_at(50, 2.6), y_at(12, 2.6), 2.6], [x_at(30, 2.6), y_at(52, 2.6), 2.6]])
    near = np.array([[x_at(58, 4.0), y_at(20, 4.0), 4.0], [x_at(62, 4.0), y_at(44, 4.0), 4.0], [0.05, 0.02, -1.0]])
    tris = np.concatenate([dense[:TIE_LO], tie[None], dense[TIE_LO:], tie[None], near[None]], 0)
    assert len(tris) == N_DENSE + 3 and np.array_equal(tris[TIE_LO], tris[TIE_HI])
    return _view_to_world(tris, R, T), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def _mesh_b(n=300):
    """A triangle soup: clip-plane crossers, degenerate and flat faces."""
    rng = np.random.default_rng(2)
    c = rng.uniform(-6, 6, (n, 1, 3))
    size = rng.choice([0.05, 0.5, 3.0, 30.0], (n, 1, 1), p=[0.2, 0.4, 0.3, 0.1])
    tri = (c + rng.normal(0, 1, (n, 3, 3)) * size).astype(np.float32)
    tri[:5, 2] = tri[:5, 1]
    tri[5:10, :, 1] = tri[5:10, :1, 1]
    return tri.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.fixture(scope="module")
def raster_ref():
    """The two meshes, their cameras and the oracle's images of every frame (computed once)."""
    items = []
    for mesh, poses in ((_mesh_a(), POSES_A), (_mesh_b(), POSES_B)):
        RT, cams = _cams(poses)
        want = np.stack([oraster.raster_zbuf(mesh[0], mesh[1], R, T, H, W, ocam.TAN_HALF_FOV) for R, T in RT])
        items.append(dict(mesh=mesh, RT=RT, cams=cams, want=want, verts=_dev(mesh[0]), faces=_dev(mesh[1])))
    return items


def _check_image(z, zf, want, what):
    z, zf = z.cpu().numpy(), zf.cpu().numpy()
    assert np.array_equal(z, want), f"{what}: depth differs from oracle/raster.py at {(z != want).sum()} pixels"
    hit = zf != -1
    assert np.array_equal(hit, want > 0), what
    assert np.array_equal(z[hit].view(np.uint32), (zf[hit] >> 32).astype(np.uint32)), what
    return zf & 0xFFFFFFFF, hit


def _check_mesh_a_frame0(face, hit, it):
    """What frame 0 of mesh A is there for: the coarse tile's list needs four pieces, the tie goes to the lower id, the near-plane
    crosser is drawn."""
    mesh, (R, T) = it["mesh"], it["RT"][0]
    assert not hit[:, 64:].all() and hit[:, :64].mean() > 0.2          # (the dense faces cover a good part of their coarse tile)
    only = lambda f: oraster.raster_zbuf(mesh[0], mesh[1][f:f + 1], R, T, H, W, ocam.TAN_HALF_FOV)      # noqa: E731
    z_lo, z_hi, z_near = only(TIE_LO), only(TIE_HI), only(N_DENSE + 2)
    tie = (z_lo > 0) & (z_lo == z_hi) & (it["want"][0] == z_lo)
    assert tie.sum() > 200, tie.sum()
    assert (face[tie] == TIE_LO).all(), "equal depths: the lowest face id wins"
    near_wins = (z_near > 0) & (it["want"][0] == z_near)
    assert near_wins.sum() > 10 and z_near[z_near > 0].min() < 1.0, "the face that crosses the near plane is drawn up to the clip plane"
    assert (face[near_wins] == N_DENSE + 2).all()
    late = face[hit & ~tie & ~near_wins]
    # Which entries land in which piece is up to the order of the setup's atomics.  The smallest piece holds N_DENSE - 3 HITS = 244 of
    # the list's ~1200 entries: a random 244 hold none of w distinct winners with probability (1 - 244 / 1207)^w, below 1e-9 from w = 100
    assert len(np.unique(late)) >= 100 and (late >= 3 * HITS).any(), "winners from every LDS piece"


def test_raster_single_form_equals_oracle(hip, raster_ref):
    a = raster_ref[0]
    z, zf = ho.raster_zface(a["verts"], a["faces"], a["cams"][:1], H, W)
    face, hit = _check_image(z[0], zf[0], a["want"][0], "mesh A, frame 0")
    _check_mesh_a_frame0(face, hit, a)
    z_only, _ = ho.raster_zbuf(a["verts"], a["faces"], a["cams"][:1], H, W)
    assert np.array_equal(z_only[0].cpu().numpy(), a["want"][0]), "the depth-only form"
    b = raster_ref[1]
    zb, zfb = ho.raster_zface(b["verts"], b["faces"], b["cams"], H, W)
    for f in range(3):
        _check_image(zb[f], zfb[f], b["want"][f], f"mesh B, frame {f}")
    assert (b["want"] > 0).mean() > 0.02


@pytest.mark.parametrize("F_", [1, 3])
def test_raster_group_form_equals_oracle(hip, raster_ref, F_):
    """Two items of different meshes (1207 and 300 faces: different setup and tile grids) in one launch, with 1 and with 3 frames."""
    order = raster_ref if F_ == 1 else raster_ref[::-1]
    outs = [dict(owner=_Owner(), z=torch.full((F_, H, W), -77.0, device=D), zf=torch.full((F_, H, W), 5, dtype=torch.int64, device=D))
            for _ in order]
    ho.raster_zface_batch([(o["owner"], it["verts"], it["faces"], it["cams"][:F_], o["z"], o["zf"]) for it, o in zip(order, outs)], H, W, F_)
    for it, o in zip(order, outs):
        for f in range(F_):
            face, hit = _check_image(o["z"][f], o["zf"][f], it["want"][f], f"{len(it['mesh'][1])} faces, frame {f} of {F_}")
            if it is raster_ref[0] and f == 0:
                _check_mesh_a_frame0(face, hit, it)


# ------------------------------------------------------------------ coverage
COV_BOX = ([0.0, 0.0, 0.0], [10.0, 10.0, 5.0])


def _cov_gt():
    """Threshold 1 over COV_BOX: the plan's cells are the unit cubes.  Column (i, j) of the 10 x 10 columns holds (3 i + j) % 10 points,
    all in the z cell [2, 3): a cloud point beside it walks a run of exactly that many -- every length 0 .. 2 UNROLL + 1, ten columns
    each -- plus the two corners of the box."""
    rng = np.random.default_rng(5)
    pts = [[0.0, 0.0, 0.0], [10.0, 10.0, 5.0]]
    runs = np.zeros((10, 10), int)
    for i in range(10):
        for j in range(10):
            n = (3 * i + j) % 10
            runs[i, j] = n
            for _ in range(n):
                pts.append([i + rng.uniform(0.05, 0.95), j + rng.uniform(0.05, 0.95), 2.0 + rng.uniform(0.05, 0.95)])
    assert sorted(set(runs.ravel().tolist())) == list(range(2 * UNROLL + 2))
    return np.array(pts, np.float32)


def _cov_cloud(seed, n):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(COV_BOX[0], np.float32), np.array(COV_BOX[1], np.float32)
    return rng.uniform(lo - 1.5, hi + 1.5, (n, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def cov_ref():
    gt = _cov_gt()
    k = 2 * len(gt)
    clouds = [(_cov_cloud(41, k // 3), 11), (_cov_cloud(42, 6 * k), 12), (_cov_cloud(43, k + 1), 13), (_cov_cloud(44, 40), 14)]
    want = [opl.coverage(gt, pc, seed=seed)[1] for pc, seed in clouds]
    assert len(clouds[0][0]) < k < len(clouds[2][0]) < len(clouds[1][0])
    assert all(0 < w < len(gt) for w in want) and len(set(want)) == len(want), want
    return gt, clouds, want


def test_coverage_single_form_equals_brute_force(hip, cov_ref):
    gt, clouds, want = cov_ref
    plan = ho.CoveragePlan(_dev(gt), 1.0, 2, bbox=COV_BOX)
    for rep in range(2):                                               # the second round: bumped epochs over stale stamps
        for (pc, seed), w in zip(clouds, want):
            out = torch.tensor([-5, -9], dtype=torch.int32, device=D)
            plan.count(_dev(pc), out, seed=seed)
            assert out.cpu().tolist() == [w, min(len(pc), 2 * len(gt))], (rep, len(pc), out.cpu().tolist(), w)


def test_coverage_group_form_equals_brute_force(hip, cov_ref):
    gt, clouds, want = cov_ref
    gt_d = _dev(gt)
    plans = [ho.CoveragePlan(gt_d, 1.0, 2, bbox=COV_BOX) for _ in clouds]      # a plan's stamps belong to one item of a launch
    pcs = [_dev(pc) for pc, _ in clouds]
    for rep in range(2):
        outs = [torch.tensor([-5, -9], dtype=torch.int32, device=D) for _ in clouds]
        ho.coverage_count_batch([(plan, pc, out, None, None, seed, False) for plan, pc, out, (_, seed) in zip(plans, pcs, outs, clouds)])
        got = [o.cpu().tolist() for o in outs]
        assert got == [[w, min(len(pc), 2 * len(gt))] for w, (pc, _) in zip(want, clouds)], (rep, got, want)


# ------------------------------------------------------------------ un-projection
UNPROJ_POSES = [([1.0, 3.3, -2.0], [0.0, 45.0]), ([4.0, 3.3, -2.0], [30.0, 90.0])]


def _depth_frames(seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.6, 120, (2, H, W)).astype(np.float32)            # a part beyond the 70-unit sensor range
    d[rng.random((2, H, W)) < 0.25] = -1
    return _dev(d)


def _state(cap=3000, start=9, colour=False):
    cloud = torch.zeros(cap, 3, device=D)
    cloud[:start] = 7.0
    return dict(cloud=cloud, count=torch.tensor([start], dtype=torch.int64, device=D), rgb=torch.zeros(cap, 3, device=D) if colour else None)


def _same_cloud(a, b, counts_a, counts_b, what):
    assert int(a["count"].item()) == int(b["count"].item()) > 9 + 100, what
    assert torch.equal(a["cloud"], b["cloud"]), f"{what}: the clouds differ"
    assert torch.equal(counts_a, counts_b), f"{what}: the (valid, kept) counts differ"


def test_unproject_depth_only_equals_colour_instantiation(hip):
    """The plain call and the filing call, in step with the cloud and out of step: without colours (the depth-only instantiation) and
    with an image's colours riding along (the colour instantiation), the same points at the same places."""
    _, cams = _cams(UNPROJ_POSES)
    rgb = torch.rand(2, H, W, 3, device=D)
    mk_bins = lambda: hu.CloudBins((-160.0, -160.0), (160.0, 160.0), 3000, D)      # noqa: E731
    d1, d2, d3 = _depth_frames(5), _depth_frames(6), _depth_frames(7)
    assert ho.unproject_files(d1, None)
    plain, col = _state(), _state(colour=True)
    bins_p, bins_c = mk_bins(), mk_bins()
    filed_p, filed_c = _state(start=0), _state(start=0, colour=True)
    for step, (depth, file_it) in enumerate(((d1, True), (d2, False), (d3, True))):
        c_p = ho.unproject_append(depth, None, cams, plain["cloud"], plain["count"], 0.2, 70.0, seed=60 + step).clone()
        c_c = ho.unproject_append(depth, None, cams, col["cloud"], col["count"], 0.2, 70.0, seed=60 + step, rgb=rgb, cloud_rgb=col["rgb"]).clone()
        _same_cloud(plain, col, c_p, c_c, f"plain call {step}")
        # step 0 files (in step), step 1 appends without the store, step 2 finds the store out of step and files nothing
        kw = dict(bins=bins_p) if file_it else {}
        f_p = ho.unproject_append(depth, None, cams, filed_p["cloud"], filed_p["count"], 0.2, 70.0, seed=60 + step, **kw).clone()
        kw = dict(bins=bins_c) if file_it else {}
        f_c = ho.unproject_append(depth, None, cams, filed_c["cloud"], filed_c["count"], 0.2, 70.0, seed=60 + step, rgb=rgb, cloud_rgb=filed_c["rgb"],
                                  **kw).clone()
        assert torch.equal(f_p, c_p) and torch.equal(f_c, c_p), step
        n = int(filed_p["count"].item())
        assert n == int(filed_c["count"].item()) == int(plain["count"].item()) - 9
        assert torch.equal(filed_p["cloud"][:n], plain["cloud"][9:9 + n]) and torch.equal(filed_c["cloud"], filed_p["cloud"]), step
        hp, hc = bins_p.header(), bins_c.header()
        assert hp["n_binned"] == hc["n_binned"] and hp["error"] == hc["error"] == 0 and hp["n_overflow"] == hc["n_overflow"] == 0, (step, hp, hc)
        if step == 0:
            n_first = n
            assert hp["n_binned"] == n
        else:
            assert hp["n_binned"] == n_first < n, "out of step: nothing more is filed"
    assert float((plain["cloud"][:9] - 7.0).abs().sum()) == 0.0 and float(col["rgb"][9:int(col["count"].item())].sum()) > 0


def test_unproject_group_form_depth_only_equals_colour_instantiation(hip, raster_ref):
    """Frames rendered from the dense mesh (background pixels are invalid): a group of depth-only items runs the depth-only
    instantiation, a group with one coloured item the colour instantiation for all of its items; the clouds are those of the single
    calls."""
    b = raster_ref[0]
    cams = b["cams"][:2]
    z, zf = ho.raster_zface(b["verts"], b["faces"], cams, H, W)
    assert 0.02 < float((z < 0).float().mean()) < 0.98
    noise = _depth_frames(8)
    vcol = _dev(np.random.default_rng(3).uniform(0.05, 1.0, (len(b["mesh"][0]), 3)).astype(np.float32))
    frames = [[z[0], z[1]], [noise[0], noise[1]]]
    seeds = (71, 72)

    def run(colour_first):
        sts = [_state(colour=colour_first and j == 0) for j in range(2)]
        shade = ([zf[0], zf[1]], b["verts"], b["faces"], vcol, 0.85)
        items = [(_Owner(), frames[j], cams, st["cloud"], st["count"], seeds[j], st["rgb"], shade if st["rgb"] is not None else None)
                 for j, st in enumerate(sts)]
        ho.unproject_append_batch(items, H, W, 2, gathering_factor=0.2)
        return sts, items

    plain, keep_p = run(False)
    mixed, keep_m = run(True)
    for j in range(2):
        ref = _state()
        counts = ho.unproject_append(torch.stack(frames[j]).contiguous(), None, cams, ref["cloud"], ref["count"], 0.2, 70.0, seed=seeds[j])
        n = int(ref["count"].item())
        assert n > 9 + 100 and int(counts[:, 1].sum().item()) == n - 9
        for what, sts in (("depth-only group", plain), ("group with a coloured item", mixed)):
            assert int(sts[j]["count"].item()) == n, (what, j)
            assert torch.equal(sts[j]["cloud"], ref["cloud"]), (what, j)
    c = mixed[0]["rgb"][9:int(mixed[0]["count"].item())].cpu().numpy()
    assert (c > 0).all() and (c <= 1).all() and len(np.unique(c, axis=0)) > 4          # shaded, not one constant colour
