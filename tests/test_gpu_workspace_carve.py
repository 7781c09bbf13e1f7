"""Every entry point that carves a caller's workspace (csrc/nbp_carve.h), at the smallest shapes where a carve can go wrong: the call
gets EXACTLY the bytes its size function asks for, starting 8 bytes past a 256-byte boundary inside a larger allocation whose 4 KiB
on either side hold a byte pattern.  Its results equal, bit for bit, the same call on an aligned and roomy workspace, and both guards
are intact afterwards.  The tests only look at memory they own."""
import ctypes as C

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import hipops as ho
from oracle import camera as ocam

pytestmark = pytest.mark.gpu
D = "cuda"
GUARD, PATTERN = 4096, 0xA5
VP, I, LL, U, SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_uint, C.c_size_t
F3 = C.c_float * 3
LO, HI = F3(0, 0, 0), F3(4, 3, 5)                      # the box of the metric cases


class Exact:
    """Hands out regions of exactly the bytes asked for, `skew` bytes past a 256-byte boundary, between two guards."""

    def __init__(self):
        self.regions = []

    def __call__(self, nbytes, skew=8):
        nbytes = int(nbytes)
        assert nbytes > 0
        buf = torch.full((GUARD + 256 + skew + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=D)
        start = (buf.data_ptr() + GUARD + 255) // 256 * 256 + skew - buf.data_ptr()
        self.regions.append((buf, start, nbytes))
        return buf.data_ptr() + start, nbytes

    def intact(self):
        return all(bool((buf[:start] == PATTERN).all()) and bool((buf[start + n:] == PATTERN).all()) for buf, start, n in self.regions)


class Roomy:
    """Aligned, zeroed, and twice the bytes asked for and a page more."""

    def __init__(self):
        self.keep = []

    def __call__(self, nbytes, skew=8):
        buf = torch.zeros(2 * int(nbytes) + 4096, dtype=torch.uint8, device=D)
        assert buf.data_ptr() % 256 == 0
        self.keep.append(buf)
        return buf.data_ptr(), buf.numel()


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _bits(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def _check(run):
    """run(alloc) -> the call's outputs; the same with exact, skewed, guarded workspaces as with roomy ones."""
    ref = run(Roomy())
    exact = Exact()
    got = run(exact)
    torch.cuda.synchronize()
    assert exact.regions, "the case carved nothing"
    assert len(ref) == len(got) and len(ref) > 0
    for k, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(_bits(a), _bits(b)), f"output {k} differs from the roomy workspace's"
    assert exact.intact(), "a guard around an exact workspace was written"
    return got


def _ok(rc):
    assert rc == 0, rc


# ------------------------------------------------------------------ un-projection
POSES = [([0.0, 0.0, 0.0], [0.0, 0.0]), ([1.5, -1.0, 2.0], [25.0, 140.0]), ([-2.0, 2.0, -1.0], [-40.0, 250.0]),
         ([2.5, 0.5, 2.0], [10.0, 30.0])]


def _cams(n):
    RT = [ocam.camera_RT(x, v) for x, v in POSES[:n]]
    return ho.cams12(np.stack([r for r, _ in RT]), np.stack([t for _, t in RT]))


def _depth(seed, F_, H, W):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.6, 120, (F_, H, W)).astype(np.float32)            # a part beyond the 70-unit sensor range
    d[rng.random((F_, H, W)) < 0.25] = -1
    return _dev(d)


@pytest.mark.parametrize("H,W", [(8, 12), (7, 9)], ids=["fast-8x12", "slow-7x9"])
@pytest.mark.parametrize("F_", [1, 4])
def test_unproject_append(hip, F_, H, W):
    depth, cams = _depth(3, F_, H, W), _cams(F_)

    def run(alloc):
        counts = torch.zeros(2 * F_, dtype=torch.int32, device=D)
        cloud, count = torch.zeros(512, 3, device=D), torch.zeros(1, dtype=torch.int64, device=D)
        ws, nws = alloc(hip.nbp_unproject_workspace_bytes(F_, H, W))
        _ok(hip.nbp_unproject_append_f32(depth.data_ptr(), None, cams.ctypes.data, F_, H, W, ho.TAN_HALF_FOV, 70.0, 0.5, 7,
                                         counts.data_ptr(), cloud.data_ptr(), count.data_ptr(), 512, ws, nws, None))
        return counts, cloud, count
    counts, cloud, count = _check(run)
    assert int(count.item()) == int(counts[1::2].sum()) > 0


def test_unproject_append_batch(hip):
    n, F_, H, W = 2, 2, 8, 12
    depth = [_depth(11 + r, F_, H, W) for r in range(n)]
    cams = np.stack([_cams(4)[:2], _cams(4)[2:]])                       # [n][F_][12]
    nul = _arr(VP, [None] * n)

    def run(alloc):
        counts = [torch.zeros(2 * F_, dtype=torch.int32, device=D) for _ in range(n)]
        cloud = [torch.zeros(512, 3, device=D) for _ in range(n)]
        count = [torch.zeros(1, dtype=torch.int64, device=D) for _ in range(n)]
        need = hip.nbp_unproject_workspace_bytes(F_, H, W)
        ws = [alloc(need) for _ in range(n)]
        _ok(hip.nbp_unproject_append_shaded_batch_f32(
            n, _arr(VP, [depth[r][f].data_ptr() for r in range(n) for f in range(F_)]), nul, nul, nul, nul, cams.ctypes.data, F_, H, W,
            ho.TAN_HALF_FOV, 70.0, 0.5, _arr(U, [7, 8]), 0.85, _arr(VP, [t.data_ptr() for t in counts]),
            _arr(VP, [t.data_ptr() for t in cloud]), nul, _arr(VP, [t.data_ptr() for t in count]), _arr(LL, [512] * n),
            _arr(VP, [p for p, _ in ws]), min(b for _, b in ws), None))
        return counts + cloud + count
    got = _check(run)
    assert all(int(c.item()) > 0 for c in got[2 * n:])


# ------------------------------------------------------------------ rasteriser
def _room(extra):
    """The closed 12-face room around the cameras, and `extra` more faces inside it."""
    h = 4.0
    v = [[x, y, zz] for x in (-h, h) for y in (-h, h) for zz in (-h, h)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    for k in range(extra):
        v += [[-1.0, -1.0 + k, 3.0], [1.0, -1.0 + k, 3.0], [0.0, 1.0 + k, 3.5]]
        f.append((len(v) - 3, len(v) - 2, len(v) - 1))
    return _dev(np.array(v, np.float32)), _dev(np.array(f, np.int32))


RH, RW, RF = 24, 40, 2


@pytest.mark.parametrize("extra", [0, 1], ids=["12-faces", "13-faces"])
def test_raster_zface(hip, extra):
    verts, faces = _room(extra)
    cams = _cams(RF)

    def run(alloc):
        z, zf = torch.zeros(RF, RH, RW, device=D), torch.zeros(RF, RH, RW, dtype=torch.int64, device=D)
        ws, nws = alloc(hip.nbp_raster_workspace_bytes(len(faces), RF, RH, RW, 0))
        _ok(hip.nbp_raster_zface_f32(verts.data_ptr(), len(verts), faces.data_ptr(), len(faces), cams.ctypes.data, RF, RH, RW,
                                     ho.TAN_HALF_FOV, ho.Z_CLIP, z.data_ptr(), zf.data_ptr(), ws, nws, None))
        return z, zf
    z, zf = _check(run)
    assert int((zf != -1).sum()) > RF * RH * RW // 2 and int((z > 0).sum()) > RF * RH * RW // 2      # the cameras are inside a closed room


def test_raster_zface_batch(hip):
    meshes = [_room(0), _room(1)]
    cams = np.stack([_cams(4)[:2], _cams(4)[2:]])

    def run(alloc):
        z = [torch.zeros(RF, RH, RW, device=D) for _ in meshes]
        zf = [torch.zeros(RF, RH, RW, dtype=torch.int64, device=D) for _ in meshes]
        ws = [alloc(hip.nbp_raster_workspace_bytes(len(f), RF, RH, RW, 0)) for _, f in meshes]
        _ok(hip.nbp_raster_zface_batch_f32(
            2, _arr(VP, [v.data_ptr() for v, _ in meshes]), _arr(I, [len(v) for v, _ in meshes]), _arr(VP, [f.data_ptr() for _, f in meshes]),
            _arr(I, [len(f) for _, f in meshes]), cams.ctypes.data, RF, RH, RW, ho.TAN_HALF_FOV, ho.Z_CLIP,
            _arr(VP, [t.data_ptr() for t in z]), _arr(VP, [t.data_ptr() for t in zf]), _arr(VP, [p for p, _ in ws]),
            _arr(SZ, [b for _, b in ws]), None))
        return z + zf
    got = _check(run)
    assert all(int((t != -1).sum()) > RF * RH * RW // 2 for t in got[2:])


def test_raster_rgbz_with_a_contrast_change(hip):
    verts, faces = _room(1)
    colors = _dev(np.random.default_rng(5).uniform(0.05, 1.0, (len(verts), 3)).astype(np.float32))
    cams = _cams(RF)

    def run(alloc):
        z, rgb = torch.zeros(RF, RH, RW, device=D), torch.zeros(RF, RH, RW, 3, device=D)
        ws, nws = alloc(hip.nbp_raster_rgb_workspace_bytes(len(faces), RF, RH, RW))
        _ok(hip.nbp_raster_rgbz_f32(verts.data_ptr(), len(verts), faces.data_ptr(), len(faces), colors.data_ptr(), cams.ctypes.data, RF,
                                    RH, RW, ho.TAN_HALF_FOV, ho.Z_CLIP, 0.85, 1.5, z.data_ptr(), rgb.data_ptr(), ws, nws, None))
        return z, rgb
    z, rgb = _check(run)
    assert int((z > 0).sum()) > RF * RH * RW // 2 and float(rgb.std()) > 0


# ------------------------------------------------------------------ coverage
def _points(seed, n, lo=(0, 0, 0), hi=(4, 3, 5)):
    return _dev(np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32))


def test_coverage_count(hip):
    gt, pc = _points(1, 50), _points(2, 200)

    def run(alloc):
        out = torch.zeros(2, dtype=torch.int32, device=D)
        ws, nws = alloc(hip.nbp_coverage_workspace_bytes(LO, HI, 1.0, 100))
        _ok(hip.nbp_coverage_count_f32(gt.data_ptr(), 50, pc.data_ptr(), 200, None, 100, 3, 1.0, LO, HI, out.data_ptr(),
                                       out[1:].data_ptr(), ws, nws, None))
        return (out,)
    out, = _check(run)
    assert 0 < int(out[0]) <= 50 and int(out[1]) == 100


def test_coverage_plan_build_and_planned_count(hip):
    gt, pc = _points(1, 50), _points(2, 200)

    def run(alloc):
        out = torch.zeros(2, dtype=torch.int32, device=D)
        plan, nplan = alloc(hip.nbp_coverage_plan_bytes(LO, HI, 1.0, 50))
        ws, nws = alloc(hip.nbp_coverage_plan_workspace_bytes(LO, HI, 1.0, 50))
        _ok(hip.nbp_coverage_plan_build_f32(gt.data_ptr(), 50, 1.0, LO, HI, plan, nplan, ws, nws, None))
        _ok(hip.nbp_coverage_count_planned_f32(plan, 50, 1.0, LO, HI, pc.data_ptr(), 200, None, 100, 3, 1, out.data_ptr(),
                                               out[1:].data_ptr(), None))
        return (out,)
    out, = _check(run)
    assert 0 < int(out[0]) <= 50 and int(out[1]) == 100


# ------------------------------------------------------------------ shell-walk grids
def test_nn_dist2(hip):
    target, query = _points(3, 50), _points(4, 64)

    def run(alloc):
        d2 = torch.zeros(64, device=D)
        ws, nws = alloc(hip.nbp_nn_dist2_workspace_bytes(LO, HI, 1.0, 50))
        _ok(hip.nbp_nn_dist2_f32(query.data_ptr(), 64, None, target.data_ptr(), 50, None, LO, HI, 2.0, 1.0, d2.data_ptr(), ws, nws, None))
        return (d2,)
    d2, = _check(run)
    assert 0 < float(d2.min()) and float(d2.max()) <= 4.0 and float(d2.min()) < 4.0


def test_mesh_plan_build_and_query(hip):
    h = np.array([4, 3, 5], np.float32)
    v = np.array([[x, y, zz] for x in (0.5, 3.5) for y in (0.5, 2.5) for zz in (0.5, 4.5)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    verts, faces = _dev(v), _dev(np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32))
    assert bool((v < h).all())
    query = _points(6, 16)

    def run(alloc):
        totals, d2 = torch.zeros(2, dtype=torch.int64, device=D), torch.zeros(16, device=D)
        plan, nplan = alloc(hip.nbp_mesh_plan_bytes(LO, HI, 1.0, 12))
        ws, nws = alloc(hip.nbp_mesh_plan_workspace_bytes(LO, HI, 1.0))
        head = (verts.data_ptr(), 8, faces.data_ptr(), 12, LO, HI, 1.0, plan)
        _ok(hip.nbp_mesh_plan_count_f32(*head, nplan, totals.data_ptr(), ws, nws, None))
        n_entries = int(totals[0].item())
        entries = torch.zeros(n_entries, dtype=torch.int32, device=D)
        _ok(hip.nbp_mesh_plan_fill_i32(*head, entries.data_ptr(), n_entries, ws, nws, None))
        _ok(hip.nbp_mesh_dist2_planned_f32(plan, entries.data_ptr(), LO, HI, 1.0, 2.0, query.data_ptr(), 16, None, d2.data_ptr(), None))
        return totals, d2
    totals, d2 = _check(run)
    assert totals.tolist()[1] == 12 and totals.tolist()[0] >= 12 and float(d2.min()) < 4.0


# ------------------------------------------------------------------ scene store
def test_scene_fill_and_coverage(hip):
    box6, grid3 = _arr(C.c_float, [0, 0, 0, 4, 3, 5]), _arr(I, [2, 2, 2])
    cap, pts = 16, _points(8, 100)

    def run(alloc):
        store, count = torch.zeros(8, cap, 3, device=D), torch.zeros(8, dtype=torch.int32, device=D)
        cov = torch.zeros(2, dtype=torch.int32, device=D)
        ws, nws = alloc(hip.nbp_scene_fill_workspace_bytes(box6, grid3, cap, 100, 0.5))
        _ok(hip.nbp_scene_fill_cells_f32(pts.data_ptr(), 100, None, box6, grid3, cap, 0.5, 0, 9, store.data_ptr(), count.data_ptr(), ws, nws,
                                         None))
        ws2, nws2 = alloc(hip.nbp_scene_coverage_workspace_bytes(box6, grid3, cap, 0.5))
        _ok(hip.nbp_scene_coverage_f32(store.data_ptr(), count.data_ptr(), cap, store.data_ptr(), count.data_ptr(), cap, box6, grid3, 0.5,
                                       cov.data_ptr(), ws2, nws2, None))
        return store, count, cov
    store, count, cov = _check(run)
    assert 0 < int(count.sum()) <= 100 and int(count.max()) <= cap
    assert cov.tolist() == [int(count.sum())] * 2                          # a store covers itself


# ------------------------------------------------------------------ cloud bins
def test_cloud_bins_init_and_a_binned_map_build(hip):
    lo2, hi2 = _arr(C.c_float, [-10, -10]), _arr(C.c_float, [10, 10])
    N, S = 1000, 64
    pts = _points(10, N, (-10, 0, -10), (10, 4, 10))
    geom, tile = (I * 3)(), (C.c_float * 3)()
    _ok(hip.nbp_cloud_bins_geometry(lo2, hi2, N, geom, tile))
    bounds = _arr(C.c_float, [0.0, 1.0, 2.0, 3.0])

    def run(alloc):
        out6 = torch.zeros(6, S, S, device=D)
        store, nstore = alloc(hip.nbp_cloud_bins_bytes(lo2, hi2, N), skew=0)       # (a store is 256-byte aligned by contract)
        _ok(hip.nbp_cloud_bins_init(store, nstore, lo2, hi2, N, None))
        _ok(hip.nbp_step_maps_binned_f32(store, geom[2], pts.data_ptr(), N, None, 0.5, 2.0, -0.5, bounds, 4, 1.9, 2.1, S, -40.0, 40.0, None, 0,
                                         None, 0, out6.data_ptr(), None, None))
        return (out6,)
    out6, = _check(run)
    assert float(out6[:5].sum()) == N
