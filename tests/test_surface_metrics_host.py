"""The definition of the cloud-to-mesh accuracy metrics (utility/surface_metrics.py, numpy): the vectorised functions against their
scalar transcriptions, closed-form cases, the fp32 error against float64, the grid walk's exit rule against brute force, the
options, the summaries, and the gather (parallel_rollout.gather_surface), on the host."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import surface_cases as cases
from nextbestpath_amd.utility import recon_metrics as rm
from nextbestpath_amd.utility import surface_metrics as sm

f32 = np.float32
# the worst |sqrt(d2_fp32) - sqrt(d2_fp64)| measured on the CPU over 200 000 cases per family is 33.5 units of
# 2^-24 (|p - a| + max(|ab|, |ac|)) (the sliver family); the bound is twice that
C_BOUND = 67.0


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---- vectorised against scalar
def test_point_triangle_vectorised_equals_the_scalar_transcription():
    fam = cases.families(np.random.default_rng(3), 150)
    fam["long"] = cases.long_slivers_on_face(np.random.default_rng(4), 150)
    for name, (p, a, b, c) in fam.items():
        got = sm.point_triangle_d2(p, a, b, c)
        want = np.array([sm.point_triangle_d2_scalar(p[i], a[i], b[i], c[i]) for i in range(len(p))], f32)
        assert got.dtype == f32 and np.array_equal(_bits(got), _bits(want)), name


def test_mesh_reference_vectorised_equals_nested_loops():
    verts, faces = cases.random_mesh(5, 23, 6.0, 2.0)
    verts[4] = np.nan                                                  # a NaN vertex, a vertex outside the box, a bad index
    verts[10] = [100, 0, 0]
    faces = np.concatenate([faces, [[0, 1, 69]], [[-1, 1, 2]]]).astype(np.int32)
    lo, hi = [-3, -3, -3], [9, 9, 9]
    q = cases.queries(6, verts, faces, lo, hi, 2.0, 1.0, 60)
    got = sm.mesh_dist2_reference(q, verts, faces, lo, hi, 2.0, chunk=100)
    assert np.array_equal(_bits(got), _bits(sm.mesh_dist2_reference_scalar(q, verts, faces, lo, hi, 2.0)))
    assert np.array_equal(_bits(got), _bits(sm.mesh_dist2_reference(q, verts, faces, lo, hi, 2.0)))          # any chunk
    assert sm.participating(verts, faces, lo, hi).tolist() == [True, False] + [True] * 1 + [False] + [True] * 19 + [False, False]


# ---- known answers
A, B, C = [0, 0, 0], [4, 0, 0], [0, 4, 0]


def _d2(p, a=A, b=B, c=C):
    return float(sm.point_triangle_d2(np.asarray(p, f32), np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)))


@pytest.mark.parametrize("h", [0.3, 1.0, 0.02, 7.7])
def test_above_the_interior_is_the_height_squared(h):
    assert _d2([1, 1, h]) == float(f32(h) * f32(h)) == _d2([1, 1, -h])


def test_on_a_vertex_an_edge_and_the_face_is_zero():
    for p in (A, B, C, [2, 0, 0], [0, 1.5, 0], [2, 2, 0], [1, 1, 0], [0.25, 3.5, 0]):
        assert _d2(p) == 0.0, p


def test_beyond_an_edge_and_beyond_a_vertex():
    assert _d2([2, -3, 0]) == 9.0                                      # beyond edge ab, in the plane
    assert _d2([2, -3, 4]) == 25.0                                     # ... and above it
    assert _d2([-3, -4, 0]) == 25.0                                    # beyond vertex a
    assert _d2([7, 0, 4]) == 25.0                                      # beyond vertex b
    assert _d2([3, 3, 0]) == 2.0                                       # beyond the hypotenuse: (1, 1) / sqrt 2 twice over


def test_degenerate_triangles_are_a_point_or_a_segment():
    assert _d2([1, 2, 2], A, A, A) == 9.0                              # a point
    assert _d2([2, 3, 0], A, B, B) == 9.0 and _d2([2, 3, 0], A, A, B) == 9.0          # a segment, either vertex doubled
    assert _d2([2, 3, 0], A, B, [2, 0, 0]) == 9.0 and _d2([6, 0, 0], A, B, [1, 0, 0]) == 4.0      # three points on a line
    assert _d2([2, 3, 0], A, B, [8, 0, 0]) == 9.0
    for p in ([1, 2, 2], [2, 3, 0]):
        assert np.isfinite(_d2(p, A, A, A)) and np.isfinite(_d2(p, A, B, B))


def test_mesh_reference_rules():
    verts = np.array([A, B, C, [0, 0, 2], [4, 0, 2], [0, 4, 2], [np.nan, 0, 0], [50, 0, 0], [np.inf, 1, 1]], f32)
    base = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    lo, hi, cap = [-5, -5, -5], [9, 9, 9], 3.0
    q = np.array([[1, 1, 0.5], [1, 1, 1.75], [1, 1, -1], [1, 1, 30], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, 0]], f32)
    want = np.array([0.25, 0.0625, 1.0, 9.0, 9.0, 9.0, 0.0], f32)
    assert np.array_equal(sm.mesh_dist2_reference(q, verts, base, lo, hi, cap), want)
    # a duplicated triangle changes nothing; triangles with a NaN, an out-of-box or an infinite vertex, or an index out of range,
    # do not take part -- each would be at distance 0 of some query otherwise
    more = np.concatenate([base, base[:1], [[6, 1, 2]], [[0, 7, 2]], [[0, 1, 8]], [[0, 1, 9]], [[-1, 1, 2]]]).astype(np.int32)
    assert np.array_equal(sm.mesh_dist2_reference(q, verts, more, lo, hi, cap), want)
    assert sm.participating(verts, more, lo, hi).tolist() == [True, True, True, False, False, False, False, False]
    # nothing participates: cap2 everywhere
    assert np.array_equal(sm.mesh_dist2_reference(q, verts, more[3:], lo, hi, cap), np.full(len(q), 9.0, f32))
    assert np.array_equal(sm.mesh_dist2_reference(q, verts, base, [5, 5, 5], [9, 9, 9], cap), np.full(len(q), 9.0, f32))
    assert sm.mesh_dist2_reference(q[:0], verts, base, lo, hi, cap).shape == (0,)


def test_mesh_box_holds_every_finite_vertex():
    verts = np.array([[1, 2, 3], [-4, 0.5, 9], [np.nan, 0, 0], [0, np.inf, 0]], f32)
    lo, hi = sm.mesh_box(verts, 2.5)
    assert lo.dtype == f32 and lo.tolist() == [-6.5, -2.0, 0.5] and hi.tolist() == [3.5, 4.5, 11.5]
    with pytest.raises(ValueError):
        sm.mesh_box(verts[2:], 1.0)


# ---- fp32 against float64
def test_fp32_error_against_float64_over_the_families():
    fam = cases.families(np.random.default_rng(2026), 4000)
    for name, v in fam.items():
        nan, worst, units = cases.error_in_units(*v)
        print(f"{name}: NaN {nan}, worst |d32 - d64| {worst:.3e}, in units of 2^-24 (|p - a| + max(|ab|, |ac|)): {units:.2f}")
        assert nan == 0 and units <= C_BOUND, name


# ---- the grid walk's exit rule
@pytest.mark.parametrize("seed,n_tri,extent,edge,cell,cap", [
    (0, 4, 0.2, 0.1, 0.5, 0.3), (1, 12, 1.5, 1.0, 1.0, 1.0), (2, 40, 6.0, 1.0, 2.0, 5.0), (3, 90, 12.0, 3.0, 1.0, 5.0),
    (4, 355, 30.0, 2.0, 2.0, 1.0), (5, 200, 30.0, 12.0, 1.0, 0.3), (6, 30, 4.0, 6.0, 0.5, 5.0), (7, 150, 20.0, 0.4, 1.0, 1.0),
    (8, 60, 9.0, 2.0, 0.5, 1.0), (9, 7, 3.0, 3.0, 2.0, 0.3), (10, 120, 15.0, 5.0, 2.0, 5.0), (11, 300, 25.0, 1.0, 0.5, 0.3)])
def test_grid_walk_equals_brute_force(seed, n_tri, extent, edge, cell, cap):
    verts, faces = cases.random_mesh(100 + seed, n_tri, extent, edge)
    lo, hi = sm.mesh_box(verts, cap)
    q = cases.queries(200 + seed, verts, faces, lo, hi, cap, cell, 300)
    # (queries up to 3 cap outside the grid as well)
    q[::7] = (np.asarray(lo) + (np.asarray(hi) - lo) * np.random.default_rng(seed).uniform(-0.5, 1.5, (len(q[::7]), 3))).astype(f32)
    want = sm.mesh_dist2_reference(q, verts, faces, lo, hi, cap)
    got = cases.walk_reference(q, verts, faces, lo, hi, cap, cell)
    assert np.array_equal(_bits(got), _bits(want))
    assert (want < f32(cap) * f32(cap)).sum() > 20 and (want == f32(cap) * f32(cap)).sum() > 5
    used, entries = sm.plan_counts(verts, faces, lo, hi, cell)
    assert used == n_tri and entries >= n_tri


# ---- options and summaries
def test_option_spec():
    assert sm.option_spec(None) is None and sm.option_spec(False) is None
    assert sm.option_spec(True) == {"thresholds": (0.05, 0.1, 0.25, 0.5, 1.0), "cap": 5.0, "cell": 1.0} == sm.option_spec({})
    assert sm.option_spec({"thresholds": [0.5], "cap": 2, "cell": 0.5}) == {"thresholds": (0.5,), "cap": 2.0, "cell": 0.5}
    for bad in ("all", 3, {"curve": True}, {"thresholds": []}, {"thresholds": [0.1] * 9}, {"thresholds": [0.0]}, {"thresholds": [-1]},
                {"thresholds": [float("nan")]}, {"thresholds": [float("inf")]}, {"thresholds": [6.0]}, {"thresholds": 3},
                {"cap": 0}, {"cap": float("inf")}, {"cell": -1}, {"thresholds": [1.0], "cap": 0.5}):
        with pytest.raises(ValueError, match="surface"):
            sm.option_spec(bad)


def test_pack_and_summarise_round_trip():
    ths = (0.1, 1.0)
    d2 = np.array([0.0, 0.0025, 0.04, 4.0, 25.0], f32)
    sums, counts = rm.stats_reference(d2, ths)
    raw = sm.pack_raw(sums, counts, len(d2))
    assert raw.dtype == np.float64 and raw.shape == (sm.RAW_HEAD + 2,)
    block = sm.summarise_raw(raw, ths, 5.0)
    assert block == {"n_points": 5, "cap": 5.0, "accuracy_mean": float(np.sqrt(d2.astype(np.float64)).sum()) / 5,
                     "accuracy_rmse": float(np.sqrt(d2.astype(np.float64).sum() / 5)),
                     "thresholds": [{"threshold": 0.1, "precision": 2 / 5}, {"threshold": 1.0, "precision": 3 / 5}]}
    json.dumps(block, allow_nan=False)
    empty = sm.summarise_raw(sm.pack_raw([0, 0], [0, 0], 0), ths, 5.0)
    assert empty["accuracy_mean"] is None and empty["accuracy_rmse"] is None
    assert [r["precision"] for r in empty["thresholds"]] == [None, None]
    json.dumps(empty, allow_nan=False)
    with pytest.raises(ValueError):
        sm.summarise_raw(raw[:-1], ths, 5.0)
    spec = sm.option_spec({"thresholds": ths})
    mesh = {"faces": 12, "faces_used": 11, "entries": 40}
    rec = sm.summarise_record(sm.pack_record(raw, None, mesh), spec)
    assert rec == {"cloud": block, "mesh": mesh, "options": {"thresholds": [0.1, 1.0], "cap": 5.0, "cell": 1.0}}
    rec = sm.summarise_record(sm.pack_record(raw, sm.pack_raw([0, 0], [0, 0], 0), mesh), spec)
    assert rec["fused"] == empty and rec["cloud"] == block
    json.dumps(rec, allow_nan=False)
    with pytest.raises(ValueError):
        sm.summarise_record(sm.pack_record(raw, None, mesh)[1:], spec)


def test_reference_on_a_box():
    verts, faces = cases.box_mesh(2.0, 0.5)
    cloud = np.concatenate([cases.points_on_mesh(1, verts, faces, 50), [[1, 1, 2.5]], [[1, 1, 50]]]).astype(f32)
    got = sm.reference(cloud, verts, faces, (0.1, 1.0), cap=3.0)
    assert got["n_points"] == 52 and got["thresholds"][0]["precision"] == 50 / 52 and got["thresholds"][1]["precision"] == 51 / 52
    assert abs(got["accuracy_mean"] - 3.5 / 52) < 1e-6


# ---- the gather
THRESHOLDS = (0.05, 0.5, 1.0)
SPEC = {"thresholds": THRESHOLDS, "cap": 5.0, "cell": 1.0}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raw(rid):
    """Run rid's record row: counts beyond 2^24 and sums that fp32 would not carry; odd runs have a fused cloud."""
    rng = np.random.default_rng(rid)
    n = 20_000_000 + rid
    cloud = sm.pack_raw(rng.uniform(0, 1e6, 2) + 1e-9, rng.integers(0, n, 3), n)
    fused = sm.pack_raw(rng.uniform(0, 1e4, 2) + 1e-9, rng.integers(0, 70_000, 3), 70_001 + rid) if rid % 2 else None
    return sm.pack_record(cloud, fused, {"faces": 2 ** 25 + rid, "faces_used": 2 ** 25 - rid, "entries": 2 ** 30 + 3 * rid})


def _worker(rank, world, port, n_runs, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    runs = [(i, 0) for i in range(n_runs)]
    results = [{"run_id": runs.index(run), "surface_raw": _raw(runs.index(run)).tolist()} for run in reversed(pr.shard(runs, r, w))]
    q.put((r, pr.gather_surface(results, runs, r, w, torch.device("cpu"), SPEC)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gather_surface_world2():
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
    assert got[1] == {}                        # the ratios are formed on rank 0 alone
    assert sorted(got[0]) == list(range(n_runs))
    for rid, block in got[0].items():
        assert block == sm.summarise_record(_raw(rid), SPEC)          # float64 all the way: equal, not close
        assert block["cloud"]["n_points"] == 20_000_000 + rid and ("fused" in block) == bool(rid % 2)
        assert block["mesh"] == {"faces": 2 ** 25 + rid, "faces_used": 2 ** 25 - rid, "entries": 2 ** 30 + 3 * rid}
        assert block["options"] == {"thresholds": list(THRESHOLDS), "cap": 5.0, "cell": 1.0}


def test_gather_surface_single_process():
    from nextbestpath_amd import parallel_rollout as pr
    res = [{"run_id": i, "surface_raw": _raw(i).tolist()} for i in range(2)]
    out = pr.gather_surface(res, [(0, 0), (1, 0)], 0, 1, torch.device("cpu"), SPEC)
    assert out == {i: sm.summarise_record(_raw(i), SPEC) for i in range(2)}
    assert pr.gather_surface(res, [(0, 0), (1, 0)], 1, 1, torch.device("cpu"), SPEC) == {}
