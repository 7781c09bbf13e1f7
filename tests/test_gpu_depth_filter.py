"""GPU: the depth-frame filter (csrc/nbp_depth_filter.hip) against its definition (utility/depth_filter.py::apply), bit for bit, in
both launch forms; its exact equivariance under the image's symmetries; its refusals; and the option `depth_filter` through the
camera, the lock-step rollouts and the collectors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import depth_filter as df
from nextbestpath_amd.utility import depth_noise as dn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def specs(radius):
    """Each stage alone, every stage on (both range terms; 39/128 + 100/512 = 1/2 exactly: gate(10) = 0.5), one range term only, the
    supports at their maxima."""
    top = (2 * radius + 1) ** 2 - 1
    return {
        "smooth": dict(radius=radius, range_base=0.5),
        "reject": dict(radius=radius, range_base=0.5, smooth=False, min_support=2 * radius),
        "fill": dict(radius=radius, range_base=0.5, smooth=False, fill_support=3 * radius),
        "all": dict(radius=radius, range_base=0.3046875, range_quad=0.001953125, min_support=2 * radius, fill_support=3 * radius),
        "quad_only": dict(radius=radius, range_quad=0.00390625, min_support=1, fill_support=top // 2),
        "base_only": dict(radius=radius, range_base=0.75, min_support=top // 2, fill_support=1),
        "maxima": dict(radius=radius, range_base=0.5, min_support=top, fill_support=top),
    }


# the kernel's tile is 32 x 32 pixels (8 lanes of 4 pixels x 32 rows) with a halo of `radius`: (37, 69) has tile edges inside the
# image in both axes, a last tile of 5 rows and 5 columns, and W % 4 == 1
SHAPES = [(1, 1), (2, 3), (7, 13), (33, 100), (64, 67), (37, 69), (256, 456)]
N_KINDS = 5


def make_frame(kind, H, W, rng, T):
    """kind 0: depths drawn from {10, 10 + T, the floats either side of it, background}, T = the gate of depth 10: gate decisions
    exactly at, just under and just over the boundary, at every lane, row and tile border; 1: a step on every multiple-of-4 column and
    a frame of far depths on the image border; 2: continuous depths with 15 % holes; 3: all background; 4: all one value."""
    if kind == 0:
        at = f32(10.0) + f32(T)
        vals = np.array([10.0, at, np.nextafter(at, f32(100)), np.nextafter(at, f32(0)), -1.0], f32)
        return vals[rng.integers(0, len(vals), (H, W))]
    if kind == 1:
        z = np.where((np.arange(W) // 4) % 2 == 0, f32(10.0), f32(16.0))[None].repeat(H, 0).astype(f32)
        z[0], z[-1], z[:, 0], z[:, -1] = 30.0, 30.0, 30.0, 30.0
        return z
    if kind == 2:
        z = rng.uniform(9.5, 11.0, (H, W)).astype(f32)
        z[rng.random((H, W)) < 0.15] = -1.0
        return z
    return np.full((H, W), -1.0 if kind == 3 else 12.5, f32)


def make_frames(n, H, W, first_kind, seed, T=0.5):
    rng = np.random.default_rng(seed)
    return np.stack([make_frame((first_kind + i) % N_KINDS, H, W, rng, T) for i in range(n)])


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def gate10(spec):
    return float(df.gate(f32(10.0), df.option_spec(spec)))


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_definition(hip, H, W, radius):
    from nextbestpath_amd.utility import hipops
    smoothed = rejected = filled = 0
    for name, spec in specs(radius).items():
        raw = make_frames(N_KINDS, H, W, 0, seed=H * W + radius, T=gate10(spec))
        d_raw = torch.from_numpy(raw).cuda()
        d_out = torch.full_like(d_raw, 7.0)
        hipops.depth_filter(d_raw, d_out, spec)
        got = d_out.cpu().numpy()
        assert np.array_equal(bits(d_raw.cpu().numpy()), bits(raw))                 # the input is unchanged
        for i in range(N_KINDS):
            want = df.apply(raw[i], spec)
            bad = np.argwhere(bits(got[i]) != bits(want))
            assert len(bad) == 0, (name, i, len(bad), bad[:4].tolist(), got[i][tuple(bad[0])], want[tuple(bad[0])])
            if name == "all":
                smoothed += int(((want != raw[i]) & (want > -1) & (raw[i] > -1)).sum())
                rejected += int(((want == -1) & (raw[i] > -1)).sum())
                filled += int(((want > -1) & (raw[i] == -1)).sum())
    assert H * W < 50 or (smoothed > 0 and rejected > 0 and filled > 0), (smoothed, rejected, filled)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("H,W", [(33, 100), (64, 67)])
def test_kernel_is_exactly_d4_equivariant(hip, H, W, radius):
    """kernel(op(z)) == op(kernel(z)) bit for bit for the two flips, the transpose and a quarter turn: a halo or tile index that is
    off by one on one side only cannot pass this, whatever the frame."""
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(H + W + radius)
    z = (rng.uniform(5.0, 6.0, (H, W)) + np.where(rng.random((H, W)) < 0.1, 3.0, 0.0)).astype(f32)
    z[rng.random((H, W)) < 0.2] = -1.0
    spec = dict(radius=radius, range_base=0.2, range_quad=0.01, min_support=2 if radius == 1 else 5, fill_support=5 if radius == 1 else 14)

    def run(a):
        d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return hipops.depth_filter(d, torch.full_like(d, 7.0), spec).cpu().numpy()
    base = run(z)
    assert np.array_equal(bits(base), bits(df.apply(z, spec)))
    assert ((base == -1) & (z > -1)).any() and ((base > -1) & (z == -1)).any() and ((base != z) & (base > -1) & (z > -1)).any()
    for name, op in (("flipud", np.flipud), ("fliplr", np.fliplr), ("transpose", np.transpose), ("rot90", np.rot90)):
        assert np.array_equal(bits(run(op(z))), bits(op(base))), name


@pytest.mark.parametrize("radius", [1, 2])
def test_aligned_width_on_unaligned_pointers(hip, radius):
    """W % 4 == 0 but the frames start 4 bytes off the 16-byte grid: the 4-byte path, the same bits, and the words around the
    output keep their value."""
    from nextbestpath_amd.utility import hipops
    H, W, n = 33, 100, 2
    spec = specs(radius)["all"]
    raw = make_frames(n, H, W, 0, seed=8, T=gate10(spec))
    want = np.stack([df.apply(raw[i], spec) for i in range(n)])
    for off_r, off_o in ((0, 0), (1, 0), (0, 1), (3, 2)):
        buf_r, buf_o = torch.zeros(n * H * W + 4, device="cuda"), torch.full((n * H * W + 4,), 7.0, device="cuda")
        d_raw, d_out = buf_r[off_r:off_r + n * H * W].view(n, H, W), buf_o[off_o:off_o + n * H * W].view(n, H, W)
        d_raw.copy_(torch.from_numpy(raw))
        hipops.depth_filter(d_raw, d_out, spec)
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(want)), (off_r, off_o)
        rest = torch.cat((buf_o[:off_o], buf_o[off_o + n * H * W:]))
        assert bool((rest == 7.0).all())


@pytest.mark.parametrize("H,W", [(7, 13), (33, 100)])
@pytest.mark.parametrize("group", [1, 3, 12, 13])
def test_batch_equals_single_calls(hip, H, W, group):
    """Ragged items: 1 to 4 frames each, frames scattered over a pool; both radii."""
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(group)
    pool = 4 * group + 3
    for radius in (1, 2):
        spec = specs(radius)["all"]
        raw = make_frames(pool, H, W, 0, seed=group, T=gate10(spec))
        d_raw = torch.from_numpy(raw).cuda()
        d_out = torch.full_like(d_raw, 7.0)
        slots = rng.permutation(pool)
        items, flat, k = [], [], 0
        for g in range(group):
            nf = 1 + (g + group) % 4
            mine = [int(s) for s in slots[k:k + nf]]
            k += nf
            items.append(([d_raw[s] for s in mine], [d_out[s] for s in mine]))
            flat += mine
        hipops.depth_filter_batch(items, spec)
        got = d_out.cpu().numpy()
        single = torch.empty(1, H, W, device="cuda")
        for s in flat:
            hipops.depth_filter(d_raw[s:s + 1], single, spec)
            assert np.array_equal(bits(got[s]), bits(single[0].cpu().numpy())), s
            assert np.array_equal(bits(got[s]), bits(df.apply(raw[s], spec))), s
        for s in set(range(pool)) - set(flat):
            assert (got[s] == 7.0).all()
        assert np.array_equal(bits(d_raw.cpu().numpy()), bits(raw))
        # the same frames as device pointers
        d_out2 = torch.full_like(d_raw, 7.0)
        shift = d_out2.data_ptr() - d_out.data_ptr()
        ptr_items = [([t.data_ptr() for t in r], [o.data_ptr() + shift for o in outs]) for r, outs in items]
        hipops.depth_filter_batch(ptr_items, spec, H, W)
        assert torch.equal(d_out, d_out2)


def test_refusals_write_nothing(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    H, W, n = 8, 12, 3
    raw = torch.from_numpy(make_frames(n, H, W, 2, seed=1)).cuda()
    before = raw.clone()
    out = torch.full_like(raw, 7.0)
    par = (1, 0.5, 0.001, 1, 2, 3)                 # radius, range_base, range_quad, smooth, min_support, fill_support
    r, o = raw.data_ptr(), out.data_ptr()
    ARG, SHAPE = -1, -3
    single = [(r, r, n, H, W), (r, r + 4 * H * W, 2, H, W), (0, o, n, H, W), (r, 0, n, H, W), (r, o, 0, H, W), (r, o, -1, H, W),
              (r, o, n, 0, W), (r, o, n, H, -3)]
    for a, b, k, h, w in single:
        assert hip.nbp_depth_filter_f32(a, b, k, h, w, *par, None) == ARG, (a == b, k, h, w)
    nan = float("nan")
    bad_specs = [(0, 0.5, 0.0, 1, 0, 0), (3, 0.5, 0.0, 1, 0, 0), (-1, 0.5, 0.0, 1, 0, 0),                 # radius
                 (1, -0.1, 0.5, 1, 0, 0), (1, 0.5, -0.1, 1, 0, 0), (1, nan, 0.5, 1, 0, 0), (1, 0.5, nan, 1, 0, 0),
                 (1, 0.0, 0.0, 1, 0, 0),                                                                  # both ranges 0
                 (1, 0.5, 0.0, 1, -1, 0), (1, 0.5, 0.0, 1, 9, 0), (1, 0.5, 0.0, 1, 0, -1), (1, 0.5, 0.0, 1, 0, 9),
                 (2, 0.5, 0.0, 1, 25, 0), (2, 0.5, 0.0, 1, 0, 25)]
    for bad in bad_specs:
        assert hip.nbp_depth_filter_f32(r, o, n, H, W, *bad, None) == ARG, bad
    assert hip.nbp_depth_filter_f32(r, o, 65536, H, W, *par, None) == SHAPE
    assert hip.nbp_depth_filter_f32(r, o, 1, 1 << 15, (1 << 14) + 1, *par, None) == SHAPE             # H W > 2^29
    VP = C.c_void_p
    hw4 = 4 * H * W
    ra, ou = [r + i * hw4 for i in range(n)], [o + i * hw4 for i in range(n)]

    def batch(k, rs, os_, h=H, w=W, p=par):
        return hip.nbp_depth_filter_batch_f32(k, (VP * max(len(rs), 1))(*rs), (VP * max(len(os_), 1))(*os_), h, w, *p, None)
    assert batch(n, ra, [ou[0], ra[2], ou[2]]) == ARG                # an output frame is another item's raw frame
    assert batch(n, ra, [ou[0], ou[0], ou[2]]) == ARG                # two outputs on one frame
    assert batch(n, [ra[0], 0, ra[2]], ou) == ARG
    assert batch(n, ra, [ou[0], ou[1], 0]) == ARG
    assert batch(0, ra, ou) == ARG
    assert batch(n, ra, ou, h=0) == ARG
    assert batch(n, ra, ou, w=0) == ARG
    for bad in bad_specs:
        assert batch(n, ra, ou, p=bad) == ARG, bad
    assert batch(49, [r] * 49, [o] * 49) == SHAPE
    assert batch(n, ra, ou, h=1 << 15, w=(1 << 14) + 1) == SHAPE
    assert hip.nbp_depth_filter_batch_f32(n, None, (VP * n)(*ou), H, W, *par, None) == ARG
    assert hip.nbp_depth_filter_batch_f32(n, (VP * n)(*ra), None, H, W, *par, None) == ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(raw, before)
    with pytest.raises(_lib.NbpHipError):
        hipops.depth_filter(raw, raw, {"range_base": 0.5})
    with pytest.raises(ValueError):
        hipops.depth_filter(raw, out, None)
    with pytest.raises(ValueError):
        hipops.depth_filter(raw, out, {"range_base": 0.5, "min_support": 9})
    with pytest.raises(ValueError):
        hipops.depth_filter(raw, out[:2], {"range_base": 0.5})
    with pytest.raises(ValueError):
        hipops.depth_filter_batch([([raw[0]] * 5, [out[0]] * 5)], {"range_base": 0.5})
    with pytest.raises(ValueError):
        hipops.depth_filter_batch([([r], [o])], {"range_base": 0.5})                # pointers without H and W
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(raw, before)
    # and the accepted calls do write: the exact maxima of n H W are only sizes, so the small call stands for them
    assert hip.nbp_depth_filter_f32(r, o, n, H, W, *par, None) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    out.fill_(7.0)
    assert batch(n, ra, ou) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------------------------------------------- the drivers
NOISE = dict(sigma_base=0.02, sigma_quad=0.001, dropout=0.05, edge_threshold=4.0, seed=11)
FILTER = dict(range_base=0.06, range_quad=0.003, min_support=2, fill_support=6)
INERT = dict(range_base=1.0, smooth=False)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth_filter")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=10 + i, cells=6, size=4.8, height=1.2, tess=0.4, hull="shell")
    return str(d)


def _params():
    from nextbestpath_amd.testers import nbp_planning as tp
    return tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))


@pytest.fixture(scope="module")
def net():
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    m = NBP()
    m.load_state_dict(make_explorer_state_dict(9))
    return m.cuda().eval()


def _camera(dataset, params, seed, **options):
    from nextbestpath_amd.simulator import lockstep
    from nextbestpath_amd.simulator import scene as sc
    ds = sc.SceneDataset(dataset)
    dev = torch.device("cuda")
    settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
    mesh = sc.load_scene(os.path.join(ds.data_path, ds[0]["scene_name"], ds[0]["obj_name"]), params.scene_scale_factor, dev)
    return lockstep.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=seed, **options), mesh


def test_camera_frames_are_the_definitions_of_their_clean_frames(hip, dataset):
    params = _params()
    cam, mesh = _camera(dataset, params, 4, depth_noise=NOISE, depth_filter=FILTER)
    only, _ = _camera(dataset, params, 4, depth_filter=FILTER)
    ref, _ = _camera(dataset, params, 4)
    assert ref._zraw_ring is None and ref.depth_filter is None
    assert cam.depth_filter == only.depth_filter == df.option_spec(FILTER)
    assert cam._zraw_ring.shape == cam._zclean_ring.shape == cam._zbuf_ring.shape
    assert only._zclean_ring is None and only._zraw_ring.shape == only._zbuf_ring.shape
    wseed = (11 + 7919 * 4) % (1 << 32)
    checked = changed = 0

    def check_newest(n_new):
        nonlocal checked, changed
        which = list(range(-n_new, 0))
        perfect, cams_ref = ref.frames_batch(which)
        assert torch.equal(ref.frames_batch(which, raw=True)[0], perfect)      # filter off: raw is the default
        z, cams = cam.frames_batch(which)
        assert np.array_equal(cams, cams_ref)
        assert torch.equal(cam.frames_batch(which, clean=True)[0], perfect)    # the render itself is untouched
        assert torch.equal(only.frames_batch(which, clean=True)[0], perfect)
        assert torch.equal(only.frames_batch(which, raw=True)[0], perfect)     # the filter alone: raw is the render
        for w in which:
            assert torch.equal(cam._zface_ring[cam.frames[w][2]], ref._zface_ring[ref.frames[w][2]])
            assert torch.equal(only._zface_ring[only.frames[w][2]], ref._zface_ring[ref.frames[w][2]])
        first = cam.n_frames_captured - n_new
        c, got = perfect.cpu().numpy(), z.cpu().numpy()
        raw, alone = cam.frames_batch(which, raw=True)[0].cpu().numpy(), only.frames_batch(which)[0].cpu().numpy()
        for i in range(n_new):
            noisy = dn.apply(c[i], wseed, first + i, NOISE)
            assert np.array_equal(bits(raw[i]), bits(noisy)), first + i
            want = df.apply(noisy, FILTER)
            assert np.array_equal(bits(got[i]), bits(want)), first + i
            assert np.array_equal(bits(alone[i]), bits(df.apply(c[i], FILTER))), first + i
            assert (want > -1).sum() > 1000
            changed += int(not np.array_equal(want, noisy))
            checked += 1

    assert cam.n_frames_captured == 5
    check_newest(5)
    for step in range(2):
        nxt = cam.get_neighboring_poses(cam.cam_idx)[2 * step]
        for camera in (cam, only, ref):
            camera.move_and_capture(mesh, nxt)
        check_newest(4)
    assert checked == 13 and changed == 13 and cam.n_frames_captured == 13


def _state(ro, n):
    ro.finish()
    k = int(ro.st.cloud_count.item())
    return k, ro.st.cloud[:k].clone(), ro.st.coverage_counts[:n].clone(), ro.camera.cam_idx_history


def test_lockstep_group_equals_rollouts_alone_with_noise_and_filter(hip, dataset, net):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import hipops
    params, dev, n = _params(), torch.device("cuda"), 3
    ds = sc.SceneDataset(dataset)
    kw = dict(depth_noise=NOISE, depth_filter=FILTER)
    launches = []
    with torch.no_grad():
        alone = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, **kw) for k in range(3)]
        for r in alone:
            for _ in range(n):
                r.step()
        grouped = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, **kw) for k in range(3)]
        m = tp.MultiRollout(grouped, net, dev, n_groups=1)
        real = hipops.depth_filter_batch
        hipops.depth_filter_batch = lambda items, *a, **k2: (launches.append(len(items)), real(items, *a, **k2))[1]
        try:
            for _ in range(n):
                m.step()
            m.flush()
        finally:
            hipops.depth_filter_batch = real
    assert launches == [3] * n                                   # one filter launch per group and step, not one per rollout
    for a, b in zip(alone, grouped):
        ka, ca, va, ha = _state(a, n)
        kb, cb, vb, hb = _state(b, n)
        assert ka == kb and ka > 1000 and ha == hb
        assert torch.equal(ca, cb) and torch.equal(va, vb)
        assert a.camera.n_frames_captured == b.camera.n_frames_captured == 5 + 4 * n
        last = list(range(-8, 0))
        assert [f[2] for f in a.camera.frames] == [f[2] for f in b.camera.frames]
        for sel in ({}, {"clean": True}, {"raw": True}):
            assert torch.equal(a.camera.frames_batch(last, **sel)[0], b.camera.frames_batch(last, **sel)[0])
        za, zr = a.camera.frames_batch(last)[0].cpu().numpy(), a.camera.frames_batch(last, raw=True)[0].cpu().numpy()
        for i in range(8):
            assert np.array_equal(bits(za[i]), bits(df.apply(zr[i], FILTER)))
        ra, rb = tp._result(a, n), tp._result(b, n)
        assert ra == rb and ra["depth_filter"] == df.option_spec(FILTER) and ra["depth_noise"] == dn.option_spec(NOISE)


def test_option_off_and_inert_stages_change_nothing(hip, dataset, net):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, dev, n = _params(), torch.device("cuda"), 3
    ds = sc.SceneDataset(dataset)
    got = {}
    with torch.no_grad():
        for name, kw in (("plain", {}), ("none", {"depth_filter": None}), ("inert", {"depth_filter": INERT}),
                         ("filtered", {"depth_filter": FILTER}), ("noisy", {"depth_noise": NOISE}),
                         ("noisy_none", {"depth_noise": NOISE, "depth_filter": None}),
                         ("noisy_inert", {"depth_noise": NOISE, "depth_filter": INERT})):
            ro = tp.build_rollout(params, net, ds, (0, 0), dev, seed=6, **kw)
            for _ in range(n):
                ro.step()
            got[name] = (_state(ro, n), ro)

    def same(x, y):
        (k0, c0, v0, h0), (k, c, v, h) = got[x][0], got[y][0]
        return k == k0 and h == h0 and torch.equal(c, c0) and torch.equal(v, v0)
    assert got["plain"][0][0] > 1000
    assert same("plain", "none") and same("plain", "inert") and same("noisy", "noisy_none") and same("noisy", "noisy_inert")
    assert not same("plain", "filtered") and not same("plain", "noisy")          # and the filter does reach the cloud
    for name in ("plain", "none", "noisy", "noisy_none"):
        cam = got[name][1].camera
        assert cam._zraw_ring is None and cam.depth_filter is None
        assert "depth_filter" not in tp._result(got[name][1], n)
    assert got["plain"][1].camera._zclean_ring is None
    assert tp._result(got["plain"][1], n) == tp._result(got["none"][1], n)
    assert tp._result(got["noisy"][1], n) == tp._result(got["noisy_none"][1], n)
    for name, spec in (("inert", INERT), ("noisy_inert", INERT), ("filtered", FILTER)):
        cam = got[name][1].camera
        assert cam._zraw_ring is not None
        res = tp._result(got[name][1], n)
        assert res["depth_filter"] == df.option_spec(spec)
        assert set(res) - {"depth_filter"} == set(tp._result(got["plain" if name != "noisy_inert" else "noisy"][1], n))
    last = list(range(-8, 0))
    for name in ("inert", "noisy_inert"):
        cam = got[name][1].camera
        assert torch.equal(cam.frames_batch(last)[0], cam.frames_batch(last, raw=True)[0])


class _Subset:
    def __init__(self, ds, n):
        self.ds, self.n, self.data_path = ds, n, ds.data_path

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.ds[i]


def _collect(dataset, net, tmp_path, name, K, n_poses, **options):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.utility import nbp_utils as nu
    params = _params()
    params.n_poses_in_trajectory = 4
    env = nu.LogEnv(str(tmp_path / name))
    cov = []
    n = nu.trajectory_collection(params, 1, _Subset(sc.SceneDataset(dataset), 2), env, (256, 256), (64, 64), (-40, 40), net, cov, None,
                                 torch.device("cuda"), n_poses=n_poses, n_gt_points=8000, rollouts_per_gpu=K, **options)
    return n, cov, [v for _, v in env.items()] if os.path.exists(env.file) else []       # (no record yet: no file)


def test_collectors_write_identical_records_with_the_filter(hip, dataset, net, tmp_path):
    """2 scenes, serial against a group of 2, 40 poses (test_gpu_collect_lockstep's length: records are stored)."""
    n1, cov1, v1 = _collect(dataset, net, tmp_path, "serial", 1, 40, depth_noise=NOISE, depth_filter=FILTER)
    n2, cov2, v2 = _collect(dataset, net, tmp_path, "k2", 2, 40, depth_noise=NOISE, depth_filter=FILTER)
    print(f"records {n1} / {n2}, coverage after 4 poses {cov1}")
    assert n1 == n2 == len(v1) == len(v2) and n1 > 0
    assert cov1 == cov2 and len(cov1) == 2 and min(cov1) > 0.0
    for i, (a, b) in enumerate(zip(v1, v2)):
        assert a == b, f"record {i} differs"
    _, cov0, _ = _collect(dataset, net, tmp_path, "noise_only", 1, 6, depth_noise=NOISE)
    assert cov1 != cov0                                          # the collectors did see the filtered depth
