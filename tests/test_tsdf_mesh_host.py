"""Host: the fused mesh's definition (nextbestpath_amd/utility/tsdf_mesh.py) -- the option key, the vectorised function against its
nested-loop transcription bit for bit, a plane and a sphere with known answers, the record block and the PLY files -- and the float64
gather of the block over gloo."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tsdf_mesh_cases as cases
from nextbestpath_amd.utility import surface_metrics as sm
from nextbestpath_amd.utility import tsdf
from nextbestpath_amd.utility import tsdf_mesh as tm

f32 = np.float32
bits = cases.bits


# ---------------------------------------------------------------------------------------------------------------- the option
def test_option_key():
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers import record_blocks as rb
    assert tsdf.option_spec({"mesh": True}) == {"voxel": 0.25, "trunc": 1.0, "min_weight": 1, "mesh": True}
    assert tsdf.option_spec({"mesh": False}) == tsdf.option_spec(True) == {"voxel": 0.25, "trunc": 1.0, "min_weight": 1}
    for bad in (1, 0, "yes", None, [True], np.bool_(True)):
        with pytest.raises(ValueError):
            tsdf.option_spec({"mesh": bad})
    spec = tsdf.option_spec({"voxel": 0.5, "max_depth": 30, "mesh": True})
    assert spec == {"voxel": 0.5, "trunc": 1.0, "min_weight": 1, "max_depth": 30.0, "mesh": True} and tsdf.option_spec(spec) == spec
    assert list(spec)[-1] == "mesh"
    assert tsdf.resolved_options(spec, 70) == spec and tsdf.resolved_options(tsdf.option_spec({"mesh": True}), 70)["mesh"] is True
    assert tm.enabled(spec) and not tm.enabled(tsdf.option_spec(True)) and not tm.enabled(None)

    def keys(**on):
        return [b.key for b in rb.blocks_on(tp.resolve_options(**{**dict.fromkeys(tp._test_config), **on}))]
    assert keys(fusion={"mesh": True}) == ["fusion", "fusion_mesh"] and keys(fusion=True) == ["fusion"]
    assert keys(fusion={"mesh": False}, surface_metrics=True) == ["fusion", "surface"] and keys(surface_metrics=True) == ["surface"]
    assert keys(fusion={"mesh": True}, surface_metrics=True, recon_metrics=True) == ["reconstruction", "fusion", "surface", "fusion_mesh"]
    assert [b.key for b in rb.ALL_BLOCKS][-1] == "fusion_mesh" and [b.key for b in rb.ALL_BLOCKS][:-1] == [b.key for b in rb.BLOCKS]
    # the block's context: surface_metrics' options, or its defaults, and the volume's options
    block = rb.ALL_BLOCKS[-1]
    params = type("P", (), {"sensor_range": 70.0})()
    opts = tp.resolve_options(**{**dict.fromkeys(tp._test_config), "fusion": {"mesh": True}})
    assert block.context(opts, params, 3) == (sm.option_spec(True), {"voxel": 0.25, "trunc": 1.0, "min_weight": 1, "mesh": True, "max_depth": 70.0})
    opts = tp.resolve_options(**{**dict.fromkeys(tp._test_config), "fusion": {"mesh": True}, "surface_metrics": {"thresholds": [0.5], "cap": 2.0}})
    assert block.context(opts, params, 3)[0] == {"thresholds": (0.5,), "cap": 2.0, "cell": 1.0}


def test_the_committed_config_is_the_surface_config_with_the_mesh_on():
    from nextbestpath_amd.testers import nbp_planning as tp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs/test/test_via_surface.json")) as fh:
        surface = json.load(fh)
    with open(os.path.join(root, "configs/test/test_via_fused_mesh.json")) as fh:
        fused = json.load(fh)
    assert fused["_metrics"]["fusion"] == dict(surface["_metrics"]["fusion"], mesh=True)
    fused["_metrics"]["fusion"].pop("mesh")
    assert {k: v for k, v in fused.items() if k not in ("_about", "_scenes")} == {k: v for k, v in surface.items() if k not in ("_about", "_scenes")}
    assert fused["_scenes"] == dict(surface["_scenes"], results_json_name="synth_simple_fused_mesh.json")
    p = tp.load_params(os.path.join(root, "configs/test/test_via_fused_mesh.json"))
    assert tsdf.option_spec(p.fusion) == {"voxel": 0.25, "trunc": 1.0, "min_weight": 1, "mesh": True}


# ---------------------------------------------------------------------------------------------------------------- vectorised = scalar
@pytest.mark.parametrize("min_weight", cases.MIN_WEIGHTS)
@pytest.mark.parametrize("dims", cases.DIMS)
def test_vectorised_equals_scalar(dims, min_weight):
    vol, lo = cases.random_volume(dims)
    got, want = tm.mesh(vol, lo, cases.VOXEL, min_weight), tm.mesh_scalar(vol, lo, cases.VOXEL, min_weight)
    assert got.verts.dtype == f32 and got.faces.dtype == np.int32 and got.area2.dtype == f32
    assert np.array_equal(bits(got.verts), bits(want.verts)) and np.array_equal(got.faces, want.faces)
    assert np.array_equal(bits(got.area2), bits(want.area2)) and (got.quads, got.crossings) == (want.quads, want.crossings)
    assert len(got.faces) == 2 * got.quads == len(got.area2) and got.crossings == len(tsdf.extract(vol, lo, cases.VOXEL, min_weight))
    if min(dims) < 2:
        assert len(got.verts) == 0 and len(got.faces) == 0            # no cells
    # a crossing's point is extract's point, the same bits
    M, P = tm.crossings(vol, lo, cases.VOXEL, min_weight)
    keys = np.concatenate([np.flatnonzero(M[a].reshape(-1)) * 3 + a for a in range(3)])
    pts = np.concatenate([P[a].reshape(-1, 3)[M[a].reshape(-1)] for a in range(3)])
    assert np.array_equal(bits(pts[np.argsort(keys, kind="stable")]), bits(tsdf.extract(vol, lo, cases.VOXEL, min_weight)))


def _cell_counts(M):
    """Crossings per cell, from the dense crossing mask."""
    dims = M.shape[1:]
    C = tuple(d - 1 for d in dims)
    cnt = np.zeros(C, np.int64)
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for beta in (0, 1):
            for gamma in (0, 1):
                off = [0, 0, 0]
                off[b], off[c] = beta, gamma
                cnt += M[a][tuple(slice(off[d], off[d] + C[d]) for d in range(3))]
    return cnt


def test_the_large_case_shows_what_the_cases_are_there_for():
    dims = (33, 9, 65)
    vol, lo = cases.random_volume(dims)
    m = cases.random_mesh(dims, 1)
    M, _ = tm.crossings(vol, lo, cases.VOXEL, 1)
    assert m.quads > 500 and m.crossings > m.quads                      # crossings on the boundary emit nothing
    assert len(m.verts) > 2 * 2048 // 4 and int(M.sum()) == m.crossings
    # both orientations: quads whose ring was kept and quads whose ring was turned round
    S = vol[..., 0]
    neg = sum(int((M[a] & (S < 0)).sum()) for a in range(3))
    assert neg > 100 and m.crossings - neg > 100
    cnt = _cell_counts(M)
    assert int((cnt == 1).sum()) > 10 and int((cnt >= 4).sum()) > 100 and len(m.verts) == int((cnt > 0).sum())
    # unusable and saturated corners inside otherwise active cells
    use = tsdf.usable_mask(vol, 1)
    sat = (vol[..., 1] > 0) & ~use
    unseen = vol[..., 1] == 0

    def corners(mask):
        out = np.zeros(cnt.shape, bool)
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    out |= mask[di:di + cnt.shape[0], dj:dj + cnt.shape[1], dk:dk + cnt.shape[2]]
        return out
    assert int((corners(sat) & (cnt > 0)).sum()) > 10 and int((corners(unseen) & (cnt > 0)).sum()) > 10
    # min_weight 2 drops voxels seen once: another mesh
    m2 = cases.random_mesh(dims, 2)
    assert 0 < len(m2.faces) < len(m.faces)
    # cells straddle every boundary between two runs of 2048 voxels: an active cell just below it, with corners beyond it
    lin = np.arange(np.prod(dims)).reshape(dims)[:-1, :-1, :-1][cnt > 0]
    assert set(range(1, 10)) <= set(((lin + dims[1] * dims[2] + dims[2] + 1) // 2048)[(lin // 2048) != ((lin + dims[1] * dims[2] + dims[2] + 1) // 2048)].tolist())


# ---------------------------------------------------------------------------------------------------------------- the plane
def _vertices_f64(vol, lo, voxel, min_weight):
    """The definition's vertices evaluated in float64 on the same fp32 inputs (lo and voxel rounded to fp32 first), in cell order,
    with the largest number of crossings in a cell and the largest magnitude of a crossing point's coordinate."""
    M, _ = tm.crossings(vol, lo, voxel, min_weight)
    dims = vol.shape[:3]
    lo64, vx = np.asarray(lo, f32).astype(np.float64), float(f32(voxel))
    D = vol[..., 0].astype(np.float64) / np.maximum(vol[..., 1], 1)
    grid = np.stack(np.meshgrid(*[lo64[a] + (np.arange(dims[a]) + 0.5) * vx for a in range(3)], indexing="ij"), -1)
    C = tuple(d - 1 for d in dims)
    acc, cnt, big = np.zeros((*C, 3)), np.zeros(C, np.int64), 0.0
    for a in range(3):
        s0 = tuple(slice(0, -1) if b == a else slice(None) for b in range(3))
        s1 = tuple(slice(1, None) if b == a else slice(None) for b in range(3))
        P = grid.copy()
        with np.errstate(all="ignore"):
            t = np.where(M[a][s0], D[s0] / (D[s0] - D[s1]), 0.0)
        P[s0 + (a,)] += t * vx
        big = max(big, float(np.abs(P[M[a]]).max()))
        b, c = [x for x in range(3) if x != a]
        for beta in (0, 1):
            for gamma in (0, 1):
                off = [0, 0, 0]
                off[b], off[c] = beta, gamma
                sl = tuple(slice(off[d], off[d] + C[d]) for d in range(3))
                acc += np.where(M[a][sl][..., None], P[sl], 0.0)
                cnt += M[a][sl]
    active = cnt > 0
    return acc[active] / cnt[active][:, None], int(cnt.max()), big


def test_plane_known_answer():
    vol, lo = cases.plane_volume()
    assert min(cases.PLANE_DIMS) >= 8 and not (vol[..., 0] == 0).any()
    m = tm.mesh(vol, lo, cases.PLANE_VOXEL, 1)
    want, n, big = _vertices_f64(vol, lo, cases.PLANE_VOXEL, 1)
    assert len(m.verts) == len(want) > 100 and len(m.faces) > 100
    # in exact arithmetic every crossing, hence every vertex (a mean of crossings), lies on 4 x + 2 y + 8 z = 101 in index space
    idx = (want - lo.astype(np.float64)) / cases.PLANE_VOXEL - 0.5
    assert np.abs(idx @ np.array([4.0, 2.0, 8.0]) - 101.0).max() < 1e-9
    # The bound.  One coordinate of a vertex with n crossings in its cell is made with, per crossing, 2 roundings for the centre
    # ((f32(i) + 0.5) voxel, + lo), 2 for D0 and D1, 1 for D0 - D1, 1 for the quotient t, 1 for t voxel, 1 for centre + step and 1
    # for its addition into the sum: 9 n, and 1 for the division by the count: 9 n + 1.  Every rounding is at most 2^-24 relative to
    # its result, and no result is larger than the largest partial sum, n max|coordinate| (t <= 1 and voxel <= max|coordinate| keep
    # the steps below it; the division by n >= 1 amplifies nothing).  n and max|coordinate| are read off the float64 evaluation.
    bound = (9 * n + 1) * 2.0 ** -24 * n * big
    err = np.abs(m.verts.astype(np.float64) - want).max()
    print("plane: n", n, "max |coordinate|", big, "bound", bound, "error", err)
    assert 0 < bound < 1e-3 and err <= bound
    v = m.verts.astype(np.float64)
    normals = np.cross(v[m.faces[:, 1]] - v[m.faces[:, 0]], v[m.faces[:, 2]] - v[m.faces[:, 0]])
    assert (normals @ np.array([4.0, 2.0, 8.0]) > 0).all()


# ---------------------------------------------------------------------------------------------------------------- the sphere
def test_sphere_known_answer():
    """The fp32 definition's values on this case (the test prints them): the farthest vertex 0.01525 off the sphere, signed volume
    38.1461 (the sphere's: 38.79; the bounding spheres': 19.4 and 68.1), area 54.9136 against 4 pi r^2 = 55.4177."""
    vol, lo = cases.sphere_volume()
    voxel, r = cases.SPHERE_VOXEL, cases.SPHERE_R
    m = tm.mesh(vol, lo, voxel, 1)
    assert len(m.verts) == 1322 and len(m.faces) == 2640 and m.quads == m.crossings == 1320      # no crossing on the boundary
    # every directed edge once, and its reverse once: closed and consistently oriented
    f = m.faces.astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = directed[:, 0] * len(m.verts) + directed[:, 1]
    back = directed[:, 1] * len(m.verts) + directed[:, 0]
    assert len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(back))
    assert len(m.verts) - len(code) // 2 + len(m.faces) == 2                                      # V - E + F
    v = m.verts.astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float((a * np.cross(b, c)).sum() / 6.0)
    # a vertex lies inside a cell that the surface crosses (sqrt(3) voxel), and the sign is that of a quantised distance (trunc / 254)
    slack = np.sqrt(3.0) * voxel + cases.SPHERE_TRUNC / 254
    off = np.abs(np.sqrt(((v - cases.SPHERE_CENTRE) ** 2).sum(1)) - r)
    area = tm.area_of(m.area2)
    print("sphere: max |distance - r|", off.max(), "signed volume", volume, "area", area, "4 pi r^2", 4 * np.pi * r * r)
    assert off.max() <= slack
    assert 4 / 3 * np.pi * (r - slack) ** 3 <= volume <= 4 / 3 * np.pi * (r + slack) ** 3 and volume > 0
    assert area > 0


# ---------------------------------------------------------------------------------------------------------------- record and PLY
THRESHOLDS, CAP, CELL = (0.05, 0.25, 1.0), 2.0, 1.0
OPTIONS = {"voxel": 0.25, "trunc": 1.0, "min_weight": 1, "max_depth": 70.0, "mesh": True}


def _raw(rid):
    """Run rid's raw vector: counts beyond 2^24 and sums that fp32 would not carry."""
    rng = np.random.default_rng(rid)
    n_gt, n_v = 30_000_001 + 7 * rid, 20_000_000 + rid
    acc = sm.pack_raw(rng.uniform(0, 1e6, 2) + 1e-9, rng.integers(0, n_v, len(THRESHOLDS)), n_v)
    return tm.pack_raw(n_v, 2 * (n_v + 5), n_v + 5, n_v + 5 + rid, 1e5 + 1e-9 * rid, rng.uniform(0, 1e6, 2) + 1e-9,
                       rng.integers(0, n_gt, len(THRESHOLDS)), n_gt, acc)


def test_record_round_trip_and_reference_block():
    spec = {"thresholds": THRESHOLDS, "cap": CAP, "cell": CELL}
    raw = _raw(3)
    assert raw.dtype == np.float64 and raw.shape == (tm.raw_width(len(THRESHOLDS)),)
    block = tm.summarise_raw(raw, spec, OPTIONS)
    assert list(block) == ["vertices", "faces", "quads", "crossings", "area", "completeness", "accuracy", "options"]
    assert (block["vertices"], block["faces"], block["quads"], block["crossings"]) == (20_000_003, 40_000_016, 20_000_008, 20_000_011)
    assert block["area"] == raw[4] and block["options"] == {"thresholds": list(THRESHOLDS), "cap": CAP, "cell": CELL, "fusion": OPTIONS}
    comp = block["completeness"]
    assert list(comp) == ["n_gt", "cap", "completeness_mean", "completeness_rmse", "thresholds"] and comp["n_gt"] == 30_000_022
    assert comp["completeness_mean"] == raw[5] / comp["n_gt"] and comp["completeness_rmse"] == (raw[6] / comp["n_gt"]) ** 0.5
    assert comp["thresholds"] == [{"threshold": t, "recall": raw[8 + k] / comp["n_gt"]} for k, t in enumerate(THRESHOLDS)]
    assert block["accuracy"] == sm.summarise_raw(raw[8 + len(THRESHOLDS):], THRESHOLDS, CAP)
    assert json.loads(json.dumps(block, allow_nan=False)) == block and "fusion" not in tm.summarise_raw(raw, spec)["options"]
    with pytest.raises(ValueError):
        tm.summarise_raw(raw[:-1], spec)
    # the whole block from a volume: the sphere against a box around it
    vol, lo = cases.sphere_volume()
    gv, gf, gt = cases.gt_box([-2.0, -2.1, -1.9], [2.0, 2.0, 2.1], 300, seed=1)
    m = tm.mesh(vol, lo, cases.SPHERE_VOXEL, 1)
    ref = tm.reference_block(vol, lo, cases.SPHERE_VOXEL, 1, gt, gv, gf, THRESHOLDS, CAP, CELL, OPTIONS, fused=m)
    assert ref == tm.reference_block(vol, lo, cases.SPHERE_VOXEL, 1, gt, gv, gf, THRESHOLDS, CAP, CELL, OPTIONS)
    assert (ref["vertices"], ref["faces"], ref["quads"], ref["crossings"]) == (1322, 2640, 1320, 1320) and ref["area"] == tm.area_of(m.area2)
    assert ref["completeness"]["n_gt"] == 300 and ref["accuracy"]["n_points"] == 1322
    assert 0 < ref["completeness"]["completeness_mean"] < 1.6 and 0 < ref["accuracy"]["accuracy_mean"] < 1.6   # the box's corners: sqrt(12) - 2.1
    json.dumps(ref, allow_nan=False)
    # a mesh without faces: every GT point is `cap` away, exactly
    empty = tm.reference_block(tsdf.empty_volume((4, 4, 4)), lo, 0.25, 1, gt, gv, gf, THRESHOLDS, CAP, CELL)
    assert (empty["vertices"], empty["faces"], empty["area"]) == (0, 0, 0.0) and empty["accuracy"]["accuracy_mean"] is None
    assert empty["completeness"]["completeness_mean"] == float(np.sqrt(np.float64(f32(CAP) * f32(CAP)))) * 300 / 300
    assert [t["recall"] for t in empty["completeness"]["thresholds"]] == [0.0, 0.0, 0.0]
    json.dumps(empty, allow_nan=False)


def test_ply_round_trip(tmp_path):
    m = cases.random_mesh((33, 9, 65), 1)
    verts = m.verts.copy()
    verts[0] = [np.float32(-0.0), np.nextafter(f32(1), f32(2)), np.float32(1e-40)]      # a signed zero, an odd last bit, a denormal
    path = str(tmp_path / "mesh.ply")
    tm.write_ply(path, verts, m.faces)
    v, f = tm.read_ply(path)
    assert v.dtype == f32 and f.dtype == np.int32 and np.array_equal(bits(v), bits(verts)) and np.array_equal(f, m.faces)
    with open(path, "rb") as fh:
        text = fh.read(400).split(b"end_header\n")[0].decode()
    head = text.split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and f"element vertex {len(verts)}" in head
    assert "property float x" in head and "property list uchar int vertex_indices" in head and f"element face {len(m.faces)}" in head
    assert os.path.getsize(path) == len(text) + len("end_header\n") + 12 * len(verts) + 13 * len(m.faces)
    tm.write_ply(path, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    v, f = tm.read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with open(path, "ab") as fh:
        fh.write(b"x")
    with pytest.raises(ValueError):
        tm.read_ply(path)


# ---------------------------------------------------------------------------------------------------------------- the gather
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_runs, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    runs = [(i, 0) for i in range(n_runs)]
    results = [{"run_id": runs.index(run), "fusion_mesh_raw": _raw(runs.index(run)).tolist()} for run in reversed(pr.shard(runs, r, w))]
    spec = {"thresholds": THRESHOLDS, "cap": CAP, "cell": CELL}
    q.put((r, pr.gather_fusion_mesh(results, runs, r, w, torch.device("cpu"), spec, OPTIONS)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gather_fusion_mesh_world2():
    n_runs, world = 5, 2                       # odd count: rank 1 has a padded row
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_runs, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    spec = {"thresholds": THRESHOLDS, "cap": CAP, "cell": CELL}
    assert got[1] == {} and sorted(got[0]) == list(range(n_runs))                    # the ratios are formed on rank 0 alone
    for rid, block in got[0].items():
        assert block == tm.summarise_raw(_raw(rid), spec, OPTIONS)                   # float64 all the way: equal, not close
        assert block["vertices"] == 20_000_000 + rid and block["completeness"]["n_gt"] == 30_000_001 + 7 * rid
        assert block["area"] == 1e5 + 1e-9 * rid and block["options"]["fusion"] == OPTIONS


def test_gather_fusion_mesh_single_process_and_through_collect_records():
    from types import SimpleNamespace
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.testers import nbp_planning as tp
    spec = {"thresholds": THRESHOLDS, "cap": CAP, "cell": CELL}
    res = [{"run_id": i, "fusion_mesh_raw": _raw(i).tolist()} for i in range(2)]
    out = pr.gather_fusion_mesh(res, [(0, 0), (1, 0)], 0, 1, torch.device("cpu"), spec, OPTIONS)
    assert out == {i: tm.summarise_raw(_raw(i), spec, OPTIONS) for i in range(2)}
    with pytest.raises(ValueError):
        pr.gather_fusion_mesh([{"run_id": 0, "fusion_mesh_raw": _raw(0)[:-1].tolist()}], [(0, 0)], 0, 1, torch.device("cpu"), spec)
    # the tail of a test run: the block is formed from the gathered row, behind `surface`, and the raw key is gone
    opts = tp.resolve_options(**{**dict.fromkeys(tp._test_config), "fusion": {"mesh": True}, "surface_metrics": dict(spec)})
    runs = [(0, 0), (0, 1)]
    fusion_raw = tsdf.pack_raw(np.arange(8.0), 5, 4, 3)
    surface_raw = sm.pack_record(sm.pack_raw([1.0, 2.0], [1, 2, 3], 4), sm.pack_raw([1.0, 2.0], [1, 2, 3], 4), {"faces": 1, "faces_used": 1, "entries": 1})
    results = [{"scene": "s", "start": k, "coverage": [0.5, 0.75], "X_cam_history": [], "V_cam_history": [], "n_points": 1,
                "fusion": {}, "fusion_raw": fusion_raw.tolist(), "surface": {}, "surface_raw": surface_raw.tolist(),
                "fusion_mesh": {"formed_locally": k}, "fusion_mesh_raw": _raw(k).tolist()} for k in range(2)]
    gathered, out = tp.collect_records(results, runs, runs, 0, 1, torch.device("cpu"), opts, SimpleNamespace(sensor_range=70.0), 2, ["s"])
    fusion_options = tsdf.resolved_options(opts.fusion, 70.0)
    for k in range(2):
        rec = out["s"][str(k)]
        assert list(rec) == ["coverage", "auc", "fusion", "surface", "fusion_mesh", "X_cam_history", "V_cam_history"]
        assert rec["fusion_mesh"] == tm.summarise_raw(_raw(k), opts.surface_metrics, fusion_options) and "fusion_mesh_raw" not in gathered[k]
