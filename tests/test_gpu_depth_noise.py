"""GPU: the depth-sensor noise model (csrc/nbp_depth_noise.hip) against its definition (utility/depth_noise.py::apply), bit for bit,
in both launch forms; its refusals; and the option `depth_noise` through the camera, the lock-step rollouts, the random-walk rollout
and the collectors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import depth_noise as dn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
THR, Z_MIN = 5.0, 0.5
SPECS = {
    "base": dict(sigma_base=0.05),
    "quad": dict(sigma_quad=0.002),
    "dropout": dict(dropout=0.1),
    "dropout_heavy": dict(dropout=0.999),
    "edge": dict(edge_threshold=THR),
    "all": dict(sigma_base=0.01, sigma_quad=0.002, dropout=0.1, edge_threshold=THR, z_min=Z_MIN, seed=3),
}
SHAPES = [(1, 1), (7, 13), (33, 100), (64, 67), (256, 456)]


def make_frame(kind, H, W, rng):
    """kind 0: depths drawn from {10, 10 + THR, the floats next to it, a depth below z_min, background}: steps exactly at, just under
    and just over the threshold, everywhere (borders and lane boundaries included); 1: a step on every multiple-of-4 column and a
    frame of far depths on the image border; 2: continuous depths with holes; 3: all background."""
    if kind == 0:
        at = f32(10.0 + THR)
        vals = np.array([10.0, at, np.nextafter(at, f32(100)), np.nextafter(at, f32(0)), 0.25, -1.0], f32)
        return vals[rng.integers(0, len(vals), (H, W))]
    if kind == 1:
        z = np.where((np.arange(W) // 4) % 2 == 0, f32(10.0), f32(16.0))[None].repeat(H, 0).astype(f32)
        z[0], z[-1], z[:, 0], z[:, -1] = 30.0, 30.0, 30.0, 30.0
        return z
    if kind == 2:
        z = rng.uniform(0.1, 70.0, (H, W)).astype(f32)
        z[rng.random((H, W)) < 0.15] = -1.0
        return z
    return np.full((H, W), -1.0, f32)


def make_frames(n, H, W, first_kind, seed):
    rng = np.random.default_rng(seed)
    return np.stack([make_frame((first_kind + i) % 4, H, W, rng) for i in range(n)])


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_definition(hip, H, W):
    from nextbestpath_amd.utility import hipops
    combos = [(1, 0, 0), (1, 0, 3), (4, 4294967294, 0), (5, 0, 1)]
    n_dropped = n_kept = 0
    for name, spec in SPECS.items():
        for n, first, kind in combos:
            clean = make_frames(n, H, W, kind, seed=H * W + n)
            d_clean = torch.from_numpy(clean).cuda()
            d_out = torch.full_like(d_clean, 7.0)
            hipops.depth_noise(d_clean, d_out, 12345, first, spec)
            got = d_out.cpu().numpy()
            assert np.array_equal(d_clean.cpu().numpy(), clean)
            for i in range(n):
                want = dn.apply(clean[i], 12345, (first + i) % (1 << 32), spec)
                bad = np.argwhere(bits(got[i]) != bits(want))
                assert len(bad) == 0, (name, n, first, i, len(bad), bad[:4].tolist())
                n_dropped += int(((want == -1) & (clean[i] > -1)).sum())
                n_kept += int((want > -1).sum())
    assert n_kept > 0 and (H * W < 50 or n_dropped > 0)


def test_aligned_width_on_unaligned_pointers(hip):
    """W % 4 == 0 but the frames start 4 bytes off the 16-byte grid: the 4-byte path, the same bits."""
    from nextbestpath_amd.utility import hipops
    H, W, n = 33, 100, 2
    clean = make_frames(n, H, W, 0, seed=8)
    for off_c, off_o in ((1, 0), (0, 1), (3, 2)):
        buf_c, buf_o = torch.zeros(n * H * W + 4, device="cuda"), torch.full((n * H * W + 4,), 7.0, device="cuda")
        d_clean, d_out = buf_c[off_c:off_c + n * H * W].view(n, H, W), buf_o[off_o:off_o + n * H * W].view(n, H, W)
        d_clean.copy_(torch.from_numpy(clean))
        hipops.depth_noise(d_clean, d_out, 9, 17, SPECS["all"])
        got = d_out.cpu().numpy()
        for i in range(n):
            assert np.array_equal(bits(got[i]), bits(dn.apply(clean[i], 9, 17 + i, SPECS["all"])))
        rest = torch.cat((buf_o[:off_o], buf_o[off_o + n * H * W:]))
        assert bool((rest == 7.0).all())


@pytest.mark.parametrize("H,W", [(7, 13), (33, 100)])
@pytest.mark.parametrize("group", [1, 3, 12, 13])
def test_batch_equals_single_calls(hip, H, W, group):
    """Ragged items: 1 to 4 frames each, their own seeds and frame ids, frames scattered over a pool."""
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(group)
    pool = 4 * group + 3
    clean = make_frames(pool, H, W, 0, seed=group)
    d_clean = torch.from_numpy(clean).cuda()
    d_out = torch.full_like(d_clean, 7.0)
    slots = rng.permutation(pool)
    items, flat, k = [], [], 0
    for g in range(group):
        nf = 1 + (g + group) % 4
        mine = [int(s) for s in slots[k:k + nf]]
        k += nf
        seed = int(rng.integers(0, 1 << 32))
        ids = [int(v) for v in rng.integers(0, 1 << 32, nf)]
        if g == 0:
            ids[0] = 4294967295
        items.append(([d_clean[s] for s in mine], [d_out[s] for s in mine], seed, ids))
        flat += [(s, seed, f) for s, f in zip(mine, ids)]
    hipops.depth_noise_batch(items, SPECS["all"])
    got = d_out.cpu().numpy()
    single = torch.empty(1, H, W, device="cuda")
    used = set()
    for s, seed, f in flat:
        hipops.depth_noise(d_clean[s:s + 1], single, seed, f, SPECS["all"])
        assert np.array_equal(bits(got[s]), bits(single[0].cpu().numpy())), (s, seed, f)
        assert np.array_equal(bits(got[s]), bits(dn.apply(clean[s], seed, f, SPECS["all"])))
        used.add(s)
    for s in set(range(pool)) - used:
        assert (got[s] == 7.0).all()
    # the same frames as device pointers
    d_out2 = torch.full_like(d_clean, 7.0)
    hw4 = H * W * 4
    ptr_items = [([t.data_ptr() for t in c], [d_out2.data_ptr() + (o.data_ptr() - d_out.data_ptr()) // hw4 * hw4 for o in outs], seed, ids)
                 for c, outs, seed, ids in items]
    hipops.depth_noise_batch(ptr_items, SPECS["all"], H, W)
    assert torch.equal(d_out, d_out2)


def test_refusals_write_nothing(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    H, W, n = 8, 12, 3
    clean = torch.from_numpy(make_frames(n, H, W, 2, seed=1)).cuda()
    before = clean.clone()
    out = torch.full_like(clean, 7.0)
    par = (0.01, 0.002, 0.5, 1 << 28, 5.0)
    c, o = clean.data_ptr(), out.data_ptr()
    single = [(c, c, n, H, W), (c, c + 4 * H * W, 2, H, W), (0, o, n, H, W), (c, 0, n, H, W), (c, o, 0, H, W), (c, o, -1, H, W),
              (c, o, n, 0, W), (c, o, n, H, -3)]
    for a, b, k, h, w in single:
        assert hip.nbp_depth_noise_f32(a, b, k, h, w, 1, 0, *par, None) == -1, (a == b, k, h, w)
    for bad in ((-0.1, 0.0, 0.5, 0, 0.0), (0.0, float("nan"), 0.5, 0, 0.0), (0.0, 0.0, 0.0, 0, 0.0), (0.0, 0.0, 0.5, 0, -1.0)):
        assert hip.nbp_depth_noise_f32(c, o, n, H, W, 1, 0, *bad, None) == -1, bad
    VP, U = C.c_void_p, C.c_uint
    hw4 = 4 * H * W
    cl, ou = [c + i * hw4 for i in range(n)], [o + i * hw4 for i in range(n)]
    seeds, ids = (U * 64)(*range(64)), (U * 64)(*range(64))

    def batch(k, cs, os_, h=H, w=W):
        return hip.nbp_depth_noise_batch_f32(k, (VP * max(len(cs), 1))(*cs), (VP * max(len(os_), 1))(*os_), seeds, ids, h, w, *par, None)
    assert batch(n, cl, [ou[0], cl[2], ou[2]]) == -1                 # an output frame is another item's clean frame
    assert batch(n, cl, [ou[0], ou[0], ou[2]]) == -1                 # two outputs on one frame
    assert batch(n, [cl[0], 0, cl[2]], ou) == -1
    assert batch(n, cl, [ou[0], ou[1], 0]) == -1
    assert batch(0, cl, ou) == -1
    assert batch(n, cl, ou, h=0) == -1
    assert batch(n, cl, ou, w=0) == -1
    assert batch(49, [c] * 49, [o] * 49) == -3
    assert hip.nbp_depth_noise_batch_f32(n, None, (VP * n)(*ou), seeds, ids, H, W, *par, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(clean, before)
    with pytest.raises(_lib.NbpHipError):
        hipops.depth_noise(clean, clean, 1, 0, SPECS["all"])
    with pytest.raises(ValueError):
        hipops.depth_noise(clean, out, 1, 0, None)
    with pytest.raises(ValueError):
        hipops.depth_noise(clean, out, 1, 0, {"dropout": 1.0})
    assert torch.equal(clean, before)
    # and the accepted call does write
    assert hip.nbp_depth_noise_f32(c, o, n, H, W, 1, 0, *par, None) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------------------- the drivers
NOISE = dict(sigma_base=0.02, sigma_quad=0.001, dropout=0.05, edge_threshold=4.0, seed=11)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth_noise")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=10 + i, cells=6, size=4.8, height=1.2, tess=0.4, hull="shell")
    return str(d)


def _params():
    from nextbestpath_amd.testers import nbp_planning as tp
    return tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))


def _net():
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    return net.cuda().eval()


def _camera(dataset, params, seed, depth_noise):
    from nextbestpath_amd.simulator import lockstep
    from nextbestpath_amd.simulator import scene as sc
    ds = sc.SceneDataset(dataset)
    dev = torch.device("cuda")
    settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
    mesh = sc.load_scene(os.path.join(ds.data_path, ds[0]["scene_name"], ds[0]["obj_name"]), params.scene_scale_factor, dev)
    return lockstep.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=seed,
                                      depth_noise=depth_noise), mesh


def test_camera_frames_are_the_definition_of_their_clean_frames(hip, dataset):
    params = _params()
    cam, mesh = _camera(dataset, params, 4, NOISE)
    ref, _ = _camera(dataset, params, 4, None)
    assert ref._zclean_ring is None and ref.depth_noise is None
    assert cam.depth_noise == dn.option_spec(NOISE) and cam._zclean_ring.shape == cam._zbuf_ring.shape
    wseed = (11 + 7919 * 4) % (1 << 32)
    checked = 0

    def check_newest(n_new):
        nonlocal checked
        which = list(range(-n_new, 0))
        noisy, cams = cam.frames_batch(which)
        clean, _ = cam.frames_batch(which, clean=True)
        perfect, cams_ref = ref.frames_batch(which)
        assert np.array_equal(cams, cams_ref)
        assert torch.equal(clean, perfect)                       # the render itself is untouched
        assert torch.equal(ref.frames_batch(which, clean=True)[0], perfect)
        for w in which:
            assert torch.equal(cam._zface_ring[cam.frames[w][2]], ref._zface_ring[ref.frames[w][2]])
        first = cam.n_frames_captured - n_new
        c, z = clean.cpu().numpy(), noisy.cpu().numpy()
        for i in range(n_new):
            want = dn.apply(c[i], wseed, first + i, NOISE)
            assert np.array_equal(bits(z[i]), bits(want)), (first + i)
            assert (want > -1).sum() > 1000 and not np.array_equal(want, c[i])
            checked += 1

    assert cam.n_frames_captured == 5
    check_newest(5)
    for step in range(3):
        nxt = cam.get_neighboring_poses(cam.cam_idx)[2 * step]
        cam.move_and_capture(mesh, nxt)
        ref.move_and_capture(mesh, nxt)
        check_newest(4)
    assert checked == 17 and cam.n_frames_captured == 17


def _state(ro, n):
    ro.finish()
    k = int(ro.st.cloud_count.item())
    return k, ro.st.cloud[:k].clone(), ro.st.coverage_counts[:n].clone(), ro.camera.cam_idx_history


def test_lockstep_group_equals_rollouts_alone_with_noise(hip, dataset):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, net, dev, n = _params(), _net(), torch.device("cuda"), 4
    ds = sc.SceneDataset(dataset)
    launches = []
    with torch.no_grad():
        alone = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, depth_noise=NOISE) for k in range(3)]
        for r in alone:
            for _ in range(n):
                r.step()
        grouped = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, depth_noise=NOISE) for k in range(3)]
        m = tp.MultiRollout(grouped, net, dev, n_groups=1)
        from nextbestpath_amd.utility import hipops
        real = hipops.depth_noise_batch
        hipops.depth_noise_batch = lambda items, *a, **kw: (launches.append(len(items)), real(items, *a, **kw))[1]
        try:
            for _ in range(n):
                m.step()
            m.flush()
        finally:
            hipops.depth_noise_batch = real
    assert launches == [3] * n                                   # one noise launch per group and step, not one per rollout
    for a, b in zip(alone, grouped):
        ka, ca, va, ha = _state(a, n)
        kb, cb, vb, hb = _state(b, n)
        assert ka == kb and ka > 1000 and ha == hb
        assert torch.equal(ca, cb) and torch.equal(va, vb)
        assert a.camera.n_frames_captured == b.camera.n_frames_captured == 5 + 4 * n
        last = list(range(-8, 0))                                # the frames a camera keeps (the ring's slots 13-15 are never written)
        assert [f[2] for f in a.camera.frames] == [f[2] for f in b.camera.frames]
        for clean in (False, True):
            assert torch.equal(a.camera.frames_batch(last, clean=clean)[0], b.camera.frames_batch(last, clean=clean)[0])
    assert tp._result(grouped[0], n)["depth_noise"] == dn.option_spec(NOISE)


def test_option_off_and_zero_effects_change_nothing(hip, dataset):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, net, dev, n = _params(), _net(), torch.device("cuda"), 4
    ds = sc.SceneDataset(dataset)
    got = {}
    with torch.no_grad():
        for name, kw in (("plain", {}), ("none", {"depth_noise": None}), ("zero", {"depth_noise": {}}), ("noisy", {"depth_noise": NOISE})):
            ro = tp.build_rollout(params, net, ds, (0, 0), dev, seed=6, **kw)
            for _ in range(n):
                ro.step()
            got[name] = (_state(ro, n), ro)
    (k0, c0, v0, h0), plain = got["plain"]
    assert k0 > 1000
    for name in ("none", "zero"):
        (k, c, v, h), ro = got[name]
        assert k == k0 and h == h0 and torch.equal(c, c0) and torch.equal(v, v0), name
    assert plain.camera._zclean_ring is None and got["none"][1].camera._zclean_ring is None
    assert "depth_noise" not in tp._result(plain, n) and "depth_noise" not in tp._result(got["none"][1], n)
    assert got["zero"][1].camera._zclean_ring is not None
    (k, c, v, h), _ = got["noisy"]
    assert k != k0 or not torch.equal(c, c0)                     # and the noise does reach the cloud


def test_random_walk_true_coverage_reads_clean_frames(hip, tmp_path):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers.random_walk_planning import RandomWalkRollout, compute_random_walk_trajectory
    make_maze_scene(str(tmp_path / "m"), seed=3, cells=6, size=3.6, height=1.2, tess=0.3)
    params = _params()
    params.image_height, params.image_width = 128, 228
    params.n_proxy_points, params.n_gt_surface_points = 6000, 8000
    params.recompute_surface_every_n_loop, params.max_points_per_progressive_fill = 4, 3000
    dev = torch.device("cuda")
    ds = sc.SceneDataset(str(tmp_path), ["m"])
    settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
    mesh = sc.load_scene(os.path.join(str(tmp_path), "m", ds[0]["obj_name"]), params.scene_scale_factor, dev)
    runs = {}
    for name, spec in (("perfect", None), ("noisy", {"sigma_base": 0.5})):
        gt_scene, covered, surface, proxy = sc.setup_test_scenes(params, settings, mesh, dev, 0.05, seed=4)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=4, depth_noise=spec)
        ro = RandomWalkRollout(params, cam, gt_scene, surface, proxy, covered, mesh, dev, 0.05, seed=4)
        for _ in range(3):
            ro.step()
        k = int(ro.full_count.item())
        runs[name] = (ro.coverage_evolution, covered.cell_count.cpu().tolist(), cam.cam_idx_history, surface.cell_count.cpu().tolist(),
                      ro.full_pc[:k].clone())
    a, b = runs["perfect"], runs["noisy"]
    assert a[2] == b[2]                                          # the walk itself does not read depth
    assert a[1] == b[1] and sum(a[1]) > 0                        # covered scene: clean frames in both runs
    assert a[0] == b[0] and a[0][-1] > 0.0                       # ... hence the same true coverage
    assert a[4].shape != b[4].shape or not torch.equal(a[4], b[4])      # the full cloud is the sensor's
    assert a[3] != b[3]                                          # and so is the surface scene
    with pytest.raises(NotImplementedError):
        compute_random_walk_trajectory(params, None, cam, gt_scene, surface, proxy, covered, mesh, dev, use_perfect_depth_map=False)


class _Subset:
    def __init__(self, ds, n):
        self.ds, self.n, self.data_path = ds, n, ds.data_path

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.ds[i]


def _collect(dataset, tmp_path, name, K, depth_noise, n_poses=6):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.utility import nbp_utils as nu
    params = _params()
    params.n_poses_in_trajectory = 4
    env = nu.LogEnv(str(tmp_path / name))
    cov = []
    n = nu.trajectory_collection(params, 1, _Subset(sc.SceneDataset(dataset), 2), env, (256, 256), (64, 64), (-40, 40), _net(), cov, None,
                                 torch.device("cuda"), n_poses=n_poses, n_gt_points=8000, rollouts_per_gpu=K, depth_noise=depth_noise)
    return n, cov, [v for _, v in env.items()] if os.path.exists(env.file) else []       # (no record yet: no file)


@pytest.mark.parametrize("n_poses", [6, 40])
def test_collectors_write_identical_records_with_noise(hip, dataset, tmp_path, n_poses):
    """2 scenes, serial against groups of 2.  6 poses end before the first path does, so nothing is stored yet and the coverage after
    4 poses is what the two collectors are compared on; 40 poses (test_gpu_collect_lockstep's length) store records."""
    n1, cov1, v1 = _collect(dataset, tmp_path, "serial", 1, NOISE, n_poses)
    n2, cov2, v2 = _collect(dataset, tmp_path, "k2", 2, NOISE, n_poses)
    print(f"{n_poses} poses: records {n1} / {n2}, coverage after 4 poses {cov1}")
    assert n1 == n2 == len(v1) == len(v2)
    assert cov1 == cov2 and len(cov1) == 2 and min(cov1) > 0.0
    for i, (a, b) in enumerate(zip(v1, v2)):
        assert a == b, f"record {i} differs"
    if n_poses == 6:
        _, cov0, _ = _collect(dataset, tmp_path, "perfect", 1, None, n_poses)
        assert cov1 != cov0                                      # the collectors did see the sensor's depth
    else:
        assert n1 > 0
