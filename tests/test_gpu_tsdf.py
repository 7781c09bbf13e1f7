"""GPU: TSDF fusion (csrc/nbp_tsdf.hip) against its definition (utility/tsdf.py), bit for bit: both integrate forms, the extraction
(count, points in order, a capacity below the total, the empty volume, the saturated-voxel rule) and the statistics; the refusals;
and the option `fusion` through the rollout: an observer (same poses, coverage and cloud with it on), a volume that equals the
definition replayed on the frames the rollout un-projected, the lock-step group, and the record."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import tsdf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
VOXEL, TRUNC, MAX_DEPTH = 0.3, 0.75, 9.0
# no dimension a multiple of the workgroup's 256 (or of a wave's 64); 33 x 9 x 65 = 19 305 voxels: 76 workgroups, 10 extraction runs
VOLUMES = [(1, 1, 1), (3, 5, 7), (33, 9, 65)]
FRAMES = [(1, 1), (7, 13), (64, 114)]
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
FAR = 12.0                                           # the random frames' depths reach from 1.5 to beyond MAX_DEPTH


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def lattice_cam(position, azim, elev=0.0):
    from nextbestpath_amd.simulator.camera import Camera
    return Camera.cam12_of_pose(None, np.array([*position, elev, azim], f32))


def geometry(dims):
    """The volume in front of the identity camera: its near face at z = 2."""
    lo = np.array([-0.5 * dims[0] * VOXEL + 0.1, -0.5 * dims[1] * VOXEL - 0.07, 2.0], f32)
    centre = lo.astype(np.float64) + 0.5 * VOXEL * np.array(dims)
    return lo, centre


def cameras(dims):
    """Identity (outside the volume, looking into it); two lattice poses outside, looking at its centre along azimuths 45 and 315
    degrees; a lattice pose INSIDE it (at the centre, azimuth 90: half the voxels lie behind its clip plane)."""
    _, c = geometry(dims)
    d = 6.0
    out = [IDENTITY]
    for azim in (45.0, 315.0):
        a = np.deg2rad(azim)
        out.append(lattice_cam(c - d * np.array([np.sin(a), 0.0, np.cos(a)]) + np.array([0.0, 0.4, 0.0]), azim))
    out.append(lattice_cam(c, 90.0))
    return np.stack(out).astype(f32)


def random_frames(n, H, W, far, seed):
    """Depths over the volume's range of distances, mixed with -1, NaN and max_depth exactly, just under and just over."""
    rng = np.random.default_rng(seed)
    md = f32(MAX_DEPTH)
    special = np.array([-1.0, np.nan, md, np.nextafter(md, f32(0)), np.nextafter(md, f32(100))], f32)
    z = rng.uniform(1.5, far, (n, H, W)).astype(f32)
    pick = rng.random((n, H, W)) < 0.3
    z[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return z


def definition(dims, lo, frames, cams, trunc=TRUNC, max_depth=MAX_DEPTH, voxel=VOXEL):
    vol = tsdf.empty_volume(dims)
    for z, cam in zip(frames, cams):
        tsdf.integrate(vol, lo, voxel, z, cam, trunc, max_depth)
    return vol


def device_volume(dims):
    return torch.zeros(*dims, 2, dtype=torch.int32, device="cuda")


def check_extract(vol_host, d_vol, lo, voxel=VOXEL):
    from nextbestpath_amd.utility import hipops
    for mw in (1, 2):
        want = tsdf.extract(vol_host, lo, voxel, mw)
        got, total = hipops.tsdf_extract(d_vol, lo, voxel, mw)
        assert int(total.item()) == len(want) == got.shape[0]
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), mw
        st = tsdf.stats(vol_host, mw)
        assert hipops.tsdf_stats(d_vol, mw).tolist() == [st["observed_voxels"], st["usable_voxels"]]
    return len(tsdf.extract(vol_host, lo, voxel, 1))


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("dims", VOLUMES)
def test_kernels_equal_definition(hip, dims, H, W):
    from nextbestpath_amd.utility import hipops
    lo, _ = geometry(dims)
    cams = cameras(dims)
    frames = random_frames(4, H, W, FAR, seed=dims[0] * 1000 + H)
    want = definition(dims, lo, frames, cams)
    d_frames = torch.from_numpy(frames).cuda()
    # what the cases are there for, decided by the definition's own projection
    if dims == (33, 9, 65):
        from nextbestpath_amd.utility import view_metrics as vm
        centres = tsdf.voxel_centres(lo, VOXEL, dims)
        ok, row, col, _ = vm.project(centres, IDENTITY[:9], IDENTITY[9:], H, W)
        inside = ok & (row >= 0) & (row <= H - 1) & (col >= 0) & (col <= W - 1)
        assert inside.any() and (H * W == 1 or (ok & ~inside).any())                        # ... and voxels that project outside the image
        assert {0.0, float(W - 1)} <= set(col[inside].tolist())                             # on the first and the last column ...
        if H <= 7:                                                                          # ... and row (64 rows are finer than the voxels)
            assert {0.0, float(H - 1)} <= set(row[inside].tolist())
        ok_in, *_ = vm.project(centres, cams[3, :9], cams[3, 9:], H, W)
        assert ok_in.any() and (~ok_in).any()                                               # the camera inside: voxels behind its clip plane
        assert (want[..., 1] == 0).any() and (H * W == 1 or (want[..., 1] >= 3).any())      # voxels that no frame updated, and most did
    # one call with 4 consecutive frames
    v1 = device_volume(dims)
    hipops.tsdf_integrate(v1, lo, VOXEL, d_frames, cams, TRUNC, MAX_DEPTH)
    assert np.array_equal(v1.cpu().numpy(), want)
    assert torch.equal(d_frames.cpu().view(torch.int32), torch.from_numpy(frames).view(torch.int32))   # the frames are unchanged
    # 4 calls, in another order, and the frames by pointer
    v2 = device_volume(dims)
    for i in (2, 0, 3, 1):
        hipops.tsdf_integrate(v2, lo, VOXEL, d_frames[i], cams[i:i + 1], TRUNC, MAX_DEPTH)
    assert torch.equal(v1, v2)
    v3 = device_volume(dims)
    apart = [d_frames[i].clone() for i in range(4)]
    hipops.tsdf_integrate(v3, lo, VOXEL, apart, cams, TRUNC, MAX_DEPTH)
    assert torch.equal(v1, v3)
    # the batch form: one item with the 4 frames; and the frames spread over three items, each on a volume of its own (a voxel has
    # one owner in a launch), whose integer sums add up to the same bits
    v4 = device_volume(dims)
    hipops.tsdf_integrate_batch([(v4, lo, VOXEL, TRUNC, MAX_DEPTH, apart, cams)])
    assert torch.equal(v1, v4)
    parts = [device_volume(dims) for _ in range(3)]
    groups = ([0, 1], [2], [3])
    hipops.tsdf_integrate_batch([(p, lo, VOXEL, TRUNC, MAX_DEPTH, [d_frames[i] for i in g], cams[g]) for p, g in zip(parts, groups)])
    assert torch.equal(parts[0] + parts[1] + parts[2], v1)
    for p, g in zip(parts, groups):
        assert np.array_equal(p.cpu().numpy(), definition(dims, lo, frames[g], cams[g]))
    # the extraction and the statistics on this volume
    n = check_extract(want, v1, lo)
    assert n > 100 or dims != (33, 9, 65)


def test_sdf_exactly_at_and_one_ulp_either_side_of_the_truncation(hip):
    """Chosen voxels get a pixel whose depth makes sdf exactly -trunc, +trunc, and the floats either side of each (v2 from the
    definition, the pixel set with nextafter)."""
    from nextbestpath_amd.utility import hipops
    from nextbestpath_amd.utility import view_metrics as vm
    dims, (H, W) = (3, 5, 7), (7, 13)
    lo, _ = geometry(dims)
    trunc = f32(TRUNC)
    ok, row, col, v2 = vm.project(tsdf.voxel_centres(lo, VOXEL, dims), IDENTITY[:9], IDENTITY[9:], H, W)
    inside = np.flatnonzero(ok & (row >= 0) & (row <= H - 1) & (col >= 0) & (col <= W - 1))
    pixel_of = {}
    for v in inside:                                   # one voxel per pixel: each chosen voxel has a pixel of its own
        pixel_of[(int(row[v]), int(col[v]))] = v
    free = list(pixel_of.items())
    z = np.full((H, W), -1.0, f32)
    expect = {}
    for side, step in [(1, 0), (1, -1), (1, 1), (-1, 0), (-1, -1), (-1, 1)]:      # (+trunc first: fewer voxels have v2 + trunc a float)
        # a voxel for which v2 +- trunc is a float (then the subtraction d - v2 is exact: the two are within a factor of two)
        px, v = next((px, v) for px, v in free if f32(f32(v2[v] + f32(side) * trunc) - v2[v]) == f32(side) * trunc)
        free.remove((px, v))
        d = f32(v2[v] + f32(side) * trunc)
        if step:
            d = np.nextafter(d, f32(100) if step > 0 else f32(0))
            assert (f32(d - v2[v]) > f32(side) * trunc) == (step > 0) and f32(d - v2[v]) != f32(side) * trunc
        z[px] = d
        expect[v] = 0 if (side, step) == (-1, -1) else 1            # one ulp under -trunc: not integrated; everything else is
    want = definition(dims, lo, [z], [IDENTITY], max_depth=70.0)
    flat = want.reshape(-1, 2)
    for v, w in expect.items():
        assert flat[v, 1] == w, (v, flat[v])
    assert sorted(flat[list(expect), 0].tolist()) == [-127, -127, 0, 127, 127, 127]
    vol = device_volume(dims)
    hipops.tsdf_integrate(vol, lo, VOXEL, torch.from_numpy(z).cuda(), IDENTITY[None], TRUNC, 70.0)
    assert np.array_equal(vol.cpu().numpy(), want)


def test_twelve_items_of_different_geometries_in_one_launch(hip):
    from nextbestpath_amd.utility import hipops
    H, W = 7, 13
    rng = np.random.default_rng(5)
    items, wants, vols = [], [], []
    for i in range(12):
        dims = [(1, 1, 1), (3, 5, 7), (33, 9, 65), (2, 70, 3)][i % 4]
        voxel, trunc, max_depth, k = 0.2 + 0.05 * (i % 3), 0.7 + 0.1 * (i % 4), 6.0 + i, 1 + i % 4
        lo = np.array([-0.5 * dims[0] * voxel + 0.01 * i, -0.5 * dims[1] * voxel, 1.0 + 0.25 * i], f32)
        cams = np.stack([IDENTITY] + [lattice_cam(lo + 0.5 * voxel * np.array(dims) - np.array([0.0, 0.0, 5.0]), 0.0)] * 3)[:k]
        frames = rng.uniform(1.0, 1.0 + 0.25 * i + dims[2] * voxel + 3.0, (k, H, W)).astype(f32)
        frames[rng.random((k, H, W)) < 0.1] = -1.0
        vol = device_volume(dims)
        d = torch.from_numpy(frames).cuda()
        vols.append((vol, d))
        items.append((vol, lo, voxel, trunc, max_depth, [d[f] for f in range(k)], cams))
        wants.append(definition(dims, lo, frames, cams, trunc, max_depth, voxel))
    hipops.tsdf_integrate_batch(items)
    for i, ((vol, _), want) in enumerate(zip(vols, wants)):
        assert np.array_equal(vol.cpu().numpy(), want), i
    assert sum(int((w[..., 1] > 0).sum()) for w in wants) > 10_000
    # 13 items: chunks of 12 and 1
    again = [(torch.zeros_like(it[0]),) + it[1:] for it in items] + [(device_volume((3, 5, 7)),) + items[1][1:]]
    hipops.tsdf_integrate_batch(again)
    for i, (it, want) in enumerate(zip(again, wants + [wants[1]])):
        assert np.array_equal(it[0].cpu().numpy(), want), i


def test_extraction_capacity_empty_volume_and_saturated_voxels(hip):
    from nextbestpath_amd.utility import hipops
    dims = (33, 9, 65)
    lo, _ = geometry(dims)
    rng = np.random.default_rng(9)                      # saturated, unseen and ordinary voxels side by side
    Wt = rng.integers(0, 4, dims).astype(np.int32)
    S = (rng.integers(-127, 128, dims) * Wt).astype(np.int32)
    sat = rng.random(dims) < 0.2
    S[sat] = (127 * Wt * rng.choice([-1, 1], dims))[sat]
    want_vol = np.ascontiguousarray(np.stack([S, Wt], -1))
    vol = torch.from_numpy(want_vol).cuda()
    assert check_extract(want_vol, vol, lo) > 3 * 2048  # more points than one extraction run holds voxels
    want = tsdf.extract(want_vol, lo, VOXEL, 1)
    n = len(want)
    # a capacity below the total: the first rows, the whole count, and not a word beyond the buffer
    for cap in (0, 1, 777, n - 1, n, n + 5):
        guard = torch.full((n + 16, 3), 7.0, dtype=torch.float32, device="cuda")
        out, total = hipops.tsdf_extract(vol, lo, VOXEL, 1, out=guard[:cap])
        assert int(total.item()) == n
        k = min(cap, n)
        assert np.array_equal(bits(guard[:k].cpu().numpy()), bits(want[:k]))
        assert bool((guard[k:] == 7.0).all()), cap
    # the empty volume
    empty = device_volume(dims)
    guard = torch.full((8, 3), 7.0, dtype=torch.float32, device="cuda")
    _, total = hipops.tsdf_extract(empty, lo, VOXEL, 1, out=guard)
    pts, total2 = hipops.tsdf_extract(empty, lo, VOXEL, 1)
    assert int(total.item()) == int(total2.item()) == 0 and pts.shape == (0, 3) and bool((guard == 7.0).all())
    assert hipops.tsdf_stats(empty).tolist() == [0, 0]
    # the saturated-voxel rule, by hand: (S, W) pairs along k; |S| = 127 W is not usable
    line = np.array([[127, 1], [-50, 1], [126, 1], [-254, 2], [-253, 2], [10, 3], [0, 0], [-5, 1], [5, 1]], np.int32).reshape(1, 1, 9, 2)
    pts = tsdf.extract(line, [0, 0, 0], 1.0, 1)
    assert [round(float(p), 4) for p in pts[:, 2]] == [round(1.5 + 50 / 176, 4), round(4.5 + 126.5 / (126.5 + 10 / 3), 4), 8.0]
    got, total = hipops.tsdf_extract(torch.from_numpy(line).cuda(), [0, 0, 0], 1.0, 1)
    assert np.array_equal(bits(got.cpu().numpy()), bits(pts)) and int(total.item()) == 3
    assert hipops.tsdf_stats(torch.from_numpy(line).cuda(), 1).tolist() == [8, 6]
    assert hipops.tsdf_stats(torch.from_numpy(line).cuda(), 2).tolist() == [8, 2]


def test_two_runs_give_identical_bytes(hip):
    from nextbestpath_amd.utility import hipops
    dims = (33, 9, 65)
    lo, _ = geometry(dims)
    d = torch.from_numpy(random_frames(4, 64, 114, FAR, seed=4)).cuda()
    runs = []
    for _ in range(2):
        vol = device_volume(dims)
        hipops.tsdf_integrate(vol, lo, VOXEL, d, cameras(dims), TRUNC, MAX_DEPTH)
        pts, total = hipops.tsdf_extract(vol, lo, VOXEL, 1)
        runs.append((vol.cpu(), pts.cpu().view(torch.int32), int(total.item()), hipops.tsdf_stats(vol).tolist()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2:] == runs[1][2:]
    assert runs[0][2] > 100


def test_refusals_write_nothing(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    ARG, WS, SHAPE = -1, -2, -3
    dims, H, W, n = (3, 5, 7), 7, 13, 3
    nv = dims[0] * dims[1] * dims[2]
    vol = torch.full((*dims, 2), 7, dtype=torch.int32, device="cuda")
    depth = torch.full((n, H, W), 3.0, dtype=torch.float32, device="cuda")
    cams = np.stack([IDENTITY] * 4)
    lo3 = (C.c_float * 3)(-0.5, -0.5, 2.0)
    VP, F, I = C.c_void_p, C.c_float, C.c_int
    v, d, cp = vol.data_ptr(), depth.data_ptr(), cams.ctypes.data
    tan, zc = hipops.TAN_HALF_FOV, hipops.Z_CLIP

    def single(vol_=v, lo_=lo3, voxel=0.3, dm=dims, depth_=d, table=None, n_=n, cams_=cp, h=H, w=W, t=tan, z=zc, trunc=0.75, md=9.0):
        return hip.nbp_tsdf_integrate_f32(vol_, lo_, voxel, *dm, depth_, table, n_, cams_, h, w, t, z, trunc, md, None)
    table = (VP * n)(*[depth[i].data_ptr() for i in range(n)])
    for bad in (dict(vol_=None), dict(lo_=None), dict(cams_=None), dict(depth_=None), dict(table=table), dict(n_=0), dict(n_=-1),
                dict(dm=(0, 5, 7)), dict(dm=(3, 5, -1)), dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")),
                dict(h=0), dict(w=0), dict(t=0.0), dict(z=0.0), dict(trunc=0.0), dict(trunc=float("inf")), dict(md=0.0),
                dict(md=float("nan")), dict(lo_=(C.c_float * 3)(0.0, float("nan"), 0.0)),
                dict(depth_=v), dict(depth_=None, table=(VP * n)(d, v + 8, d)),          # a frame inside the volume
                dict(depth_=None, table=(VP * n)(d, 0, d))):
        assert single(**bad) == ARG, bad
    for bad in (dict(n_=65536), dict(dm=(1 << 10, 1 << 10, (1 << 8) + 1)), dict(dm=(1 << 20, 1 << 20, 1 << 20)), dict(vol_=v + 4),
                dict(h=1 << 15, w=(1 << 14) + 1)):
        assert single(**bad) == SHAPE, bad

    vols, los, vox, dm = (VP * 2)(v, 0), np.array([[-0.5, -0.5, 2.0]] * 2, np.float32), np.array([0.3, 0.3], np.float32), \
        np.array([dims, dims], np.int32)
    other = torch.full((*dims, 2), 7, dtype=torch.int32, device="cuda")
    tr, md, nf = np.array([0.75, 0.75], np.float32), np.array([9.0, 9.0], np.float32), (I * 2)(3, 1)
    frames = (VP * 8)(*([depth[i].data_ptr() for i in range(3)] + [0] + [depth[0].data_ptr()] + [0] * 3))
    cams2 = np.zeros((2, 4, 12), np.float32)
    cams2[:] = IDENTITY

    def batch(k=2, vols_=None, nf_=nf, frames_=frames, dm_=dm, tr_=tr, md_=md, vox_=vox, h=H, w=W, **null):
        vols_ = (VP * 2)(v, other.data_ptr()) if vols_ is None else vols_
        args = dict(vols=vols_, lo=los.ctypes.data, vox=vox_.ctypes.data, dm=dm_.ctypes.data, tr=tr_.ctypes.data, md=md_.ctypes.data, nf=nf_,
                    frames=frames_, cams=cams2.ctypes.data)
        args.update(null)
        return hip.nbp_tsdf_integrate_batch_f32(k, args["vols"], args["lo"], args["vox"], args["dm"], args["tr"], args["md"], args["nf"],
                                                args["frames"], args["cams"], h, w, tan, zc, None)
    for name in ("vols", "lo", "vox", "dm", "tr", "md", "nf", "frames", "cams"):
        assert batch(**{name: None}) == ARG, name
    assert batch(k=0) == ARG and batch(k=13) == SHAPE
    assert batch(vols_=(VP * 2)(v, 0)) == ARG and batch(vols_=(VP * 2)(v, v)) == ARG and batch(vols_=(VP * 2)(v, v + 8)) == ARG
    assert batch(nf_=(I * 2)(3, 0)) == ARG and batch(nf_=(I * 2)(5, 1)) == SHAPE and batch(nf_=(I * 2)(4, 1)) == ARG     # (a null 4th frame)
    assert batch(frames_=(VP * 8)(d, d, other.data_ptr(), 0, d, 0, 0, 0)) == ARG             # item 0's frame is item 1's volume
    assert batch(tr_=np.array([0.75, 0.0], np.float32)) == ARG and batch(md_=np.array([9.0, -1.0], np.float32)) == ARG
    assert batch(vox_=np.array([0.3, 0.0], np.float32)) == ARG and batch(h=0) == ARG
    assert batch(dm_=np.array([dims, (1 << 10, 1 << 10, 1 << 9)], np.int32)) == SHAPE

    pts = torch.full((64, 3), 7.0, dtype=torch.float32, device="cuda")
    total = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    nws = hip.nbp_tsdf_extract_workspace_bytes(nv)
    assert nws >= 256 + 8 and hip.nbp_tsdf_extract_workspace_bytes(0) == 0 and hip.nbp_tsdf_extract_workspace_bytes((1 << 28) + 1) == 0
    ws = torch.full((nws,), 7, dtype=torch.uint8, device="cuda")

    def extract(vol_=v, lo_=lo3, voxel=0.3, dm_=dims, mw=1, pts_=pts.data_ptr(), cap=64, total_=total.data_ptr(), ws_=ws.data_ptr(),
                nws_=nws):
        return hip.nbp_tsdf_extract_f32(vol_, lo_, voxel, *dm_, mw, pts_, cap, total_, ws_, nws_, None)
    for bad in (dict(vol_=None), dict(lo_=None), dict(total_=None), dict(ws_=None), dict(pts_=None), dict(mw=0), dict(cap=-1),
                dict(voxel=0.0), dict(dm_=(3, 0, 7)), dict(pts_=v), dict(total_=v + 8)):
        assert extract(**bad) == ARG, bad
    assert extract(nws_=nws - 1) == WS and extract(vol_=v + 4) == SHAPE and extract(total_=total.data_ptr() + 4) == SHAPE
    counts = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    sws = hip.nbp_tsdf_stats_workspace_bytes()
    wss = torch.full((sws,), 7, dtype=torch.uint8, device="cuda")
    for args, rc in (((None, nv, 1, counts.data_ptr(), wss.data_ptr(), sws), ARG), ((v, nv, 1, None, wss.data_ptr(), sws), ARG),
                     ((v, nv, 1, counts.data_ptr(), None, sws), ARG), ((v, 0, 1, counts.data_ptr(), wss.data_ptr(), sws), ARG),
                     ((v, nv, 0, counts.data_ptr(), wss.data_ptr(), sws), ARG), ((v, nv, 1, counts.data_ptr(), wss.data_ptr(), sws - 1), WS),
                     ((v + 4, nv, 1, counts.data_ptr(), wss.data_ptr(), sws), SHAPE), ((v, (1 << 28) + 1, 1, counts.data_ptr(), wss.data_ptr(), sws), SHAPE)):
        assert hip.nbp_tsdf_stats_i64(*args, None) == rc, args
    torch.cuda.synchronize()
    for t, fill in ((vol, 7), (other, 7), (pts, 7.0), (total, 7), (ws, 7), (counts, 7), (wss, 7), (depth, 3.0)):
        assert bool((t == fill).all())                              # nothing was written
    # the wrappers: CPU tensors raise, as everywhere; bad shapes are ValueErrors before anything is launched
    with pytest.raises(RuntimeError):
        hipops.tsdf_integrate(vol.cpu(), [0, 0, 0], 0.3, depth, cams[:3], 0.75, 9.0)
    with pytest.raises(RuntimeError):
        hipops.tsdf_integrate(vol, [0, 0, 0], 0.3, depth.cpu(), cams[:3], 0.75, 9.0)
    with pytest.raises(RuntimeError):
        hipops.tsdf_extract(vol.cpu(), [0, 0, 0], 0.3)
    with pytest.raises(RuntimeError):
        hipops.tsdf_stats(vol.cpu())
    with pytest.raises(RuntimeError):
        hipops.TSDFVolume(([0, 0, 0], [1, 1, 1]), tsdf.resolved_options(tsdf.option_spec(True), 70.0), "cpu")
    with pytest.raises(ValueError):
        hipops.TSDFVolume(([0, 0, 0], [1, 1, 1]), None, "cuda")
    with pytest.raises(ValueError):
        hipops.tsdf_integrate(vol, [0, 0, 0], 0.3, depth, cams[:2], 0.75, 9.0)              # 3 frames, 2 cameras
    with pytest.raises(ValueError):
        hipops.tsdf_integrate(vol[..., 0], [0, 0, 0], 0.3, depth, cams[:3], 0.75, 9.0)
    with pytest.raises(ValueError):
        hipops.tsdf_integrate_batch([(vol, [0, 0, 0], 0.3, 0.75, 9.0, [depth[0]] * 5, np.stack([IDENTITY] * 5))])
    with pytest.raises(_lib.NbpHipError):
        hipops.tsdf_integrate_batch([(vol, [0, 0, 0], 0.3, 0.75, 9.0, [depth[0]], cams[:1])] * 2)     # one volume twice in a launch
    torch.cuda.synchronize()
    assert bool((vol == 7).all())
    # and the accepted calls do write
    assert single() == 0 and batch(frames_=(VP * 8)(d, d, d, 0, d, 0, 0, 0)) == 0 and extract() == 0
    assert hip.nbp_tsdf_stats_i64(v, nv, 1, counts.data_ptr(), wss.data_ptr(), sws, None) == 0
    torch.cuda.synchronize()
    assert not bool((vol == 7).all()) and not bool((other == 7).all()) and counts.tolist()[0] == nv
    total.fill_(-1)
    assert extract() == 0 and int(total.item()) >= 0


def test_volume_object(hip):
    from nextbestpath_amd.utility import hipops
    spec = tsdf.resolved_options(tsdf.option_spec({"voxel": 0.3, "trunc": 0.75}), 9.0)
    bbox = ([-1.0, -0.5, 2.75], [1.0, 0.5, 6.0])
    tv = hipops.TSDFVolume(bbox, spec, "cuda")
    lo, dims = tsdf.volume_geometry(bbox, spec)
    assert tv.options == spec and tv.dims == tuple(dims.tolist()) and tv.lo == lo.tolist() and tv.frames == 0 and not bool(tv.vol.any())
    frames = random_frames(5, 7, 13, 9.0, seed=8)
    cams = np.stack([IDENTITY] * 5)
    d = torch.from_numpy(frames).cuda()
    tv.integrate(d[:1], cams[:1])
    hipops.tsdf_integrate_batch([tv.item([d[i] for i in range(1, 5)], cams[1:])])
    assert tv.frames == 5
    want = definition(tv.dims, lo, frames, cams, spec["trunc"], spec["max_depth"], spec["voxel"])
    assert np.array_equal(tv.vol.cpu().numpy(), want)
    pts, n = tv.extract()
    ref = tsdf.extract(want, lo, spec["voxel"], 1)
    assert n == len(ref) > 0 and np.array_equal(bits(pts.cpu().numpy()), bits(ref)) and tv.stats() == tsdf.stats(want, 1)
    tv.reset()
    assert tv.frames == 0 and not bool(tv.vol.any()) and tv.extract()[1] == 0


# ---------------------------------------------------------------------------------------------------------------- the rollout
FUSION = {"voxel": 0.5, "trunc": 1.0}
N_STEPS = 6


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth_fusion")
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


def _state(ro, n):
    ro.finish()
    k = int(ro.st.cloud_count.item())
    return k, ro.st.cloud[:k].clone(), ro.st.coverage_counts[:n].clone(), list(ro.camera.cam_idx_history)


def _replay(ro, recorded):
    """The definition applied to the frames and cameras the rollout un-projected."""
    tv = ro.fusion
    vol = tsdf.empty_volume(tv.dims)
    for depth, cams in recorded:
        for z, cam in zip(depth, cams):
            tsdf.integrate(vol, tv.lo, tv.voxel, z, cam, tv.trunc, tv.max_depth)
    return vol


def _record_frames(ro, into):
    real = ro.camera.frames_batch

    def wrapper(which, *a, **k):
        depth, cams = real(which, *a, **k)
        into.append((depth.cpu().numpy().copy(), cams.copy()))
        return depth, cams
    ro.camera.frames_batch = wrapper


@pytest.fixture(scope="module")
def runs(dataset, net):
    """6 steps of one scene with fusion off and with fusion on (the frames the second un-projects are recorded)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, dev = _params(), torch.device("cuda")
    ds = sc.SceneDataset(dataset)
    recorded = []
    with torch.no_grad():
        off = tp.build_rollout(params, net, ds, (0, 0), dev, seed=6)
        on = tp.build_rollout(params, net, ds, (0, 0), dev, seed=6, fusion=FUSION)
        _record_frames(on, recorded)
        for ro in (off, on):
            for _ in range(N_STEPS):
                ro.step()
            ro.finish()
    return params, off, on, recorded


def test_fusion_is_an_observer(hip, runs):
    """Poses, coverage counts and the cloud's bytes.  (The cloud's colours are left out: two plain rollouts of one scene and seed,
    fusion off in both, were seen to differ in the red channel of 80 of 175 080 colour rows, which is not this option's doing.)"""
    params, off, on, _ = runs
    assert off.fusion is None and off.fusion_spec is None and on.fusion is not None
    k0, c0, v0, h0 = _state(off, N_STEPS)
    k1, c1, v1, h1 = _state(on, N_STEPS)
    assert k0 == k1 > 1000 and h0 == h1 and len(h0) >= N_STEPS
    assert torch.equal(c0.view(torch.int32), c1.view(torch.int32))                      # the cloud, byte for byte
    assert torch.equal(v0, v1) and int(v0[:, 0].max()) > 0
    assert np.array_equal(off.camera.X_cam_history, on.camera.X_cam_history)
    assert on.fusion.options == tsdf.resolved_options(tsdf.option_spec(FUSION), params.sensor_range)
    with pytest.raises(RuntimeError):
        off.fused_cloud()


def test_volume_equals_the_definition_replayed(hip, runs):
    _, _, on, recorded = runs
    assert [len(c) for _, c in recorded] == [1, 4] * N_STEPS and on.fusion.frames == 5 * N_STEPS
    want = _replay(on, recorded)
    assert np.array_equal(on.fusion.vol.cpu().numpy(), want)
    assert (want[..., 1] > 0).sum() > 1000 and want[..., 1].max() > 4
    pts, n = on.fused_cloud()
    ref = tsdf.extract(want, on.fusion.lo, on.fusion.voxel, 1)
    assert n == len(ref) > 100 and np.array_equal(bits(pts.cpu().numpy()), bits(ref))


def test_record_has_fusion_exactly_when_the_option_is_on(hip, runs):
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import recon_metrics as rm
    params, off, on, recorded = runs
    r_off, r_on = tp._result(off, N_STEPS), tp._result(on, N_STEPS)
    assert "fusion" not in r_off and "fusion_raw" not in r_off
    assert set(r_on) - set(r_off) == {"fusion", "fusion_raw"} and {k: r_on[k] for k in r_off} == r_off
    block = r_on["fusion"]
    want = _replay(on, recorded)
    st = tsdf.stats(want, 1)
    assert block["n_points"] == len(tsdf.extract(want, on.fusion.lo, on.fusion.voxel, 1)) and block["frames"] == 5 * N_STEPS
    assert block["observed_voxels"] == st["observed_voxels"] and block["usable_voxels"] == st["usable_voxels"]
    assert block["options"] == on.fusion.options and block["n_gt"] == len(on.gt) and block["cap"] == rm.DEFAULT_CAP
    assert 0.0 < block["accuracy_mean"] < 1.0 and block["thresholds"][0]["precision"] > 0.5      # a surface, not a scatter
    assert block == tsdf.summarise_raw(r_on["fusion_raw"], rm.DEFAULT_THRESHOLDS, rm.DEFAULT_CAP, on.fusion.options)
    assert on.fusion_metrics() == block
    import json
    json.dumps(r_on)


def test_lockstep_group_gives_each_rollout_the_volume_it_gets_alone(hip, dataset, net):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import hipops
    params, dev, n = _params(), torch.device("cuda"), 3
    ds = sc.SceneDataset(dataset)
    launches = []
    with torch.no_grad():
        alone = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, fusion=FUSION) for k in range(3)]
        for r in alone:
            for _ in range(n):
                r.step()
        grouped = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k, fusion=FUSION) for k in range(3)]
        m = tp.MultiRollout(grouped, net, dev, n_groups=1)
        real = hipops.tsdf_integrate_batch
        hipops.tsdf_integrate_batch = lambda items, *a, **k2: (launches.append(len(items)), real(items, *a, **k2))[1]
        try:
            for _ in range(n):
                m.step()
            m.flush()
        finally:
            hipops.tsdf_integrate_batch = real
    assert launches == [3, 3] * n                                # one launch per group and frame set, not one per rollout
    for a, b in zip(alone, grouped):
        ka, ca, va, ha = _state(a, n)
        kb, cb, vb, hb = _state(b, n)
        assert ka == kb > 1000 and ha == hb and torch.equal(ca, cb) and torch.equal(va, vb)
        assert a.fusion.frames == b.fusion.frames == 5 * n and a.fusion.dims == b.fusion.dims
        assert torch.equal(a.fusion.vol, b.fusion.vol) and int((a.fusion.vol[..., 1] > 0).sum()) > 1000
        assert tp._result(a, n) == tp._result(b, n)
