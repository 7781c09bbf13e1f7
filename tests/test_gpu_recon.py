"""GPU: the reconstruction-quality metrics (csrc/nbp_recon.hip through hipops.nn_dist2 / NNPlan / recon_stats / ReconMetrics and
the rollout driver's `recon_metrics` option) against their numpy definition (utility/recon_metrics.py).

The nearest-neighbour distances must equal the brute force BIT FOR BIT (np.array_equal): the kernel evaluates the same fp32
expression on a subset of the pairs that provably holds the minimum.  Brute force stays at or below ~4 k x 6 k pairs per case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import recon_metrics as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LANES, UNROLL, BLOCK = 8, 4, 256          # csrc/nbp_recon.hip: lanes per query, points of a run per iteration, threads per block
STATS_THREADS = 256 * 256                 # ... and the summary's fixed launch: 256 blocks of 256 threads


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _count(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


# ---- nearest neighbour: the cases.  Each returns q, t, lo, hi, cap, w and optionally the device counts (n_q, n_t).
def _case_random(cap):
    rng = np.random.default_rng(11)
    t = rng.uniform(-10, 10, (6007, 3)).astype(f32)               # some outside the box
    q = rng.uniform(-13, 13, (4099, 3)).astype(f32)               # 4099: no multiple of the block's 32 queries
    return q, t, [-8, -5, -8], [8, 5, 8], cap, 1.0


def _case_single_target():
    rng = np.random.default_rng(12)
    return rng.uniform(-6, 6, (777, 3)).astype(f32), np.array([[0.3, -0.2, 1.1]], f32), [-4, -4, -4], [4, 4, 4], 2.5, 1.0


def _case_device_count_zero():
    rng = np.random.default_rng(13)
    return (rng.uniform(-3, 3, (100, 3)).astype(f32), rng.uniform(-3, 3, (50, 3)).astype(f32), [-4, -4, -4], [4, 4, 4], 2.5, 1.0,
            None, 0)


def _case_device_counts_below_rows():
    rng = np.random.default_rng(14)
    q = rng.uniform(-12, 12, (300, 3)).astype(f32)
    t = rng.uniform(-4, 4, (200, 3)).astype(f32)
    tail = np.concatenate([q[:150], np.full((30, 3), np.nan, f32)])    # beyond the count: points at distance 0, and NaNs
    return q, np.concatenate([t, tail]), [-4, -4, -4], [4, 4, 4], 6.0, 1.0, 211, 200


def _case_cell_populations():
    rng = np.random.default_rng(15)
    cells = {(2, 2, 2): 1000, (0, 0, 0): 1, (4, 1, 3): 2, (1, 4, 0): 3, (5, 5, 5): UNROLL + 1, (3, 3, 2): UNROLL, (2, 2, 3): 2 * UNROLL + 3}
    t = np.concatenate([np.array(c, f32) * f32(1.001) + rng.uniform(0.05, 0.95, (n, 3)).astype(f32) for c, n in cells.items()])
    q = rng.uniform(-1, 7, (600, 3)).astype(f32)
    return q, t, [0, 0, 0], [6, 6, 6], 6.0, 1.0


def _case_integer_lattice():
    rng = np.random.default_rng(16)
    t = rng.integers(-3, 9, (900, 3)).astype(f32)                  # on cell faces of a grid with integer lo and w = 1
    q = np.concatenate([rng.integers(-6, 12, (700, 3)).astype(f32), rng.integers(-12, 24, (700, 3)).astype(f32) / f32(2),
                        rng.uniform(-6, 12, (300, 3)).astype(f32)])
    return q, t, [-2, -2, -2], [8, 8, 8], 2.5, 1.0


def _case_box_faces():
    lo, hi = np.array([-2, -1, -3], f32), np.array([3, 2, 1], f32)
    rng = np.random.default_rng(17)
    t = []
    for a in range(3):
        for side, out in ((lo, -np.inf), (hi, np.inf)):
            p = rng.uniform(lo, hi, (20, 3)).astype(f32)
            p[:10, a] = side[a]                                        # on the face: inside
            p[10:, a] = np.nextafter(side[a], f32(out))                # one float beyond it: outside
            t.append(p)
    t.append(np.stack([lo, hi]))                                       # the corners
    q = rng.uniform(lo - 4, hi + 4, (800, 3)).astype(f32)
    return q, np.concatenate(t), lo, hi, 2.5, 1.0


def _case_queries_outside():
    rng = np.random.default_rng(18)
    lo, hi, cap = np.array([0, 0, 0], f32), np.array([6, 6, 6], f32), f32(2.5)
    t = rng.uniform(0, 6, (400, 3)).astype(f32)
    t[:150, 0] = 0.0                                                   # a populated face
    t[150:250, 2] = 6.0
    base = rng.uniform(0, 6, (60, 3)).astype(f32)
    q = []
    for off in (cap * f32(0.99), cap, np.nextafter(cap, f32(10)), cap * f32(1.01), f32(1e6), f32(1e30)):
        for a in range(3):
            for sign in (-1, 1):
                p = base.copy()
                p[:, a] = (lo[a] - off) if sign < 0 else (hi[a] + off)
                q.append(p)
    q.append(np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]], f32))        # never lower the minimum: cap2
    return np.concatenate(q), t, lo, hi, cap, 1.0


def _case_sparse(cap):
    w = f32(1.0)
    R = int(np.ceil(cap / w))
    t = np.array([[3.2, 3.1, 3.3], [16.4, 16.2, 3.7], [3.6, 16.8, 16.1]], f32)
    dirs = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [-1, 1, 1], [1, -1, 1]], np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    q = []
    for d in ((R - 0.5) * w, cap * (1 - 1e-6), cap * (1 - 1e-7), cap, cap * (1 + 1e-7), cap * (1 + 1e-6), 0.5 * w, 1.5 * w):
        for p in t:
            q.append((p.astype(np.float64) + dirs * d).astype(f32))
    return np.concatenate(q), t, [0, 0, 0], [20, 20, 20], cap, w


def _case_duplicates():
    rng = np.random.default_rng(19)
    t = rng.uniform(-3, 3, (500, 3)).astype(f32)
    t = np.concatenate([t, t[:100]])
    q = np.concatenate([t[50:250], rng.uniform(-3, 3, (100, 3)).astype(f32)])
    return q, t, [-3, -3, -3], [3, 3, 3], 2.5, 1.0


def _case_flat():
    rng = np.random.default_rng(20)
    t = rng.uniform(-5, 5, (700, 3)).astype(f32)
    t[:600, 1] = 1.5                                                   # the plane y = 1.5 = lo = hi; the other 100 are outside
    q = rng.uniform(-7, 7, (900, 3)).astype(f32)
    return q, t, [-5, 1.5, -5], [5, 1.5, 5], 2.5, 1.0


def _case_one_query():
    rng = np.random.default_rng(21)
    return rng.uniform(-1, 1, (1, 3)).astype(f32), rng.uniform(-3, 3, (300, 3)).astype(f32), [-3, -3, -3], [3, 3, 3], 6.0, 1.0


def _case_ragged_queries():
    rng = np.random.default_rng(22)
    return (rng.uniform(-6, 6, (BLOCK // LANES + 1, 3)).astype(f32), rng.uniform(-3, 3, (300, 3)).astype(f32), [-3, -3, -3], [3, 3, 3],
            2.5, 0.7)


NN_CASES = {
    "random_cap2.5": lambda: _case_random(2.5), "random_cap6": lambda: _case_random(6.0), "single_target": _case_single_target,
    "device_count_zero": _case_device_count_zero, "device_counts_below_rows": _case_device_counts_below_rows,
    "cell_populations": _case_cell_populations, "integer_lattice": _case_integer_lattice, "box_faces": _case_box_faces,
    "queries_outside": _case_queries_outside, "sparse_cap2.5": lambda: _case_sparse(f32(2.5)), "sparse_cap6": lambda: _case_sparse(f32(6.0)),
    "duplicates": _case_duplicates, "flat": _case_flat, "one_query": _case_one_query, "ragged_queries": _case_ragged_queries,
}


@pytest.mark.parametrize("name", list(NN_CASES))
def test_nn_dist2_is_the_brute_force_minimum(hip, name):
    """nn_dist2 == nn_dist2_reference bit for bit; a second call gives the same bits; the planned form agrees."""
    from nextbestpath_amd.utility import hipops
    case = NN_CASES[name]()
    q, t, lo, hi, cap, w = case[:6]
    n_q, n_t = case[6:] if len(case) > 6 else (None, None)
    Q = len(q) if n_q is None else n_q
    want = rm.nn_dist2_reference(q[:Q], t if n_t is None else t[:n_t], lo, hi, cap)
    cap2 = f32(cap) * f32(cap)
    assert want.max() <= cap2
    if name in ("device_count_zero",):
        assert np.all(want == cap2)
    elif name not in ("one_query",):
        assert (want < cap2).any() and ((want == cap2).any() or name in ("duplicates", "cell_populations"))
    if name == "duplicates":
        assert np.count_nonzero(want == 0) >= 200
    qd, td = _dev(q), _dev(t)
    kw = {"n_query_dev": None if n_q is None else _count(n_q), "n_target_dev": None if n_t is None else _count(n_t)}
    sentinel = f32(-7.0)
    runs = []
    for _ in range(2):
        out = torch.full((len(q),), float(sentinel), dtype=torch.float32, device="cuda")
        got = hipops.nn_dist2(qd, td, (lo, hi), cap, w, out=out, **kw)
        assert got is out
        runs.append(out.cpu().numpy())
    plan = hipops.NNPlan(td, (lo, hi), w, n_target_dev=kw["n_target_dev"])
    planned = plan.dist2(qd, cap, n_query_dev=kw["n_query_dev"],
                         out=torch.full((len(q),), float(sentinel), dtype=torch.float32, device="cuda")).cpu().numpy()
    bad = np.flatnonzero(runs[0][:Q].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad[:5], runs[0][bad[:5]], want[bad[:5]], q[bad[:5]])
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    assert np.array_equal(planned.view(np.uint32), runs[0].view(np.uint32))
    assert np.all(runs[0][Q:] == sentinel)                      # entries beyond the device query count are never written


def test_nn_dist2_refuses_what_it_cannot_do(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    q, t = torch.zeros(4, 3, device="cuda"), torch.zeros(5, 3, device="cuda")
    with pytest.raises(_lib.NbpHipError, match="NBP_E_SHAPE"):
        hipops.nn_dist2(q, t, ([0, 0, 0], [700, 700, 700]), 1.0, 1.0)           # 701^3 > 2^28 cells
    with pytest.raises(_lib.NbpHipError, match="NBP_E_SHAPE"):
        hipops.nn_dist2(q, t, ([0, 0, 0], [3000, 1, 1]), 1.0, 1.0)              # an axis beyond the proven 2048 cells
    with pytest.raises(_lib.NbpHipError, match="NBP_E_ARG"):
        hipops.nn_dist2(q, t, ([0, 0, 0], [1, 1, 1]), 0.0, 1.0)
    with pytest.raises(_lib.NbpHipError, match="NBP_E_ARG"):
        hipops.nn_dist2(q, t, ([0, 0, 0], [1, -1, 1]), 1.0, 1.0)
    with pytest.raises(RuntimeError):
        hipops.nn_dist2(q.cpu(), t, ([0, 0, 0], [1, 1, 1]), 1.0, 1.0)           # no CPU fallback
    assert hipops.nn_dist2(q[:0], t, ([0, 0, 0], [1, 1, 1]), 1.0, 1.0).shape == (0,)
    assert torch.equal(hipops.nn_dist2(q, t[:0], ([0, 0, 0], [1, 1, 1]), 2.0, 1.0), torch.full((4,), 4.0, device="cuda"))


# ---- the summary
@pytest.fixture(scope="module")
def stats_values():
    """Squared distances up to 25 with the values around each threshold's square among them, longer than the summary's launch."""
    rng = np.random.default_rng(31)
    n = STATS_THREADS + 4321
    v = (rng.uniform(0, 5, n).astype(f32)) ** 2
    ths = (0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0)
    k = 0
    for t in ths:
        b = rm.sq_below(t)
        for x in (b, np.nextafter(b, f32(np.inf)), f32(t) * f32(t), f32(0)):
            v[k::257][:3] = x                       # early, so that every n of the test meets some
            k += 1
    return v.astype(f32), ths


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, STATS_THREADS + 4321])
def test_recon_stats_counts_exactly_and_sums_reproducibly(hip, stats_values, n):
    from nextbestpath_amd.utility import hipops
    v, ths = stats_values
    buf = np.concatenate([v[:n], np.array([np.nan, np.inf, 1e30, 0.0] * 16, f32)])            # a poisoned tail beyond n
    d2 = _dev(buf)
    for thresholds in (ths, ths[2:3]):
        want_sums, want_counts = rm.stats_reference(v[:n], thresholds)
        got = [hipops.recon_stats(d2, thresholds, n_dev=_count(n)) for _ in range(2)]
        sums, counts = got[0][0].cpu().numpy(), got[0][1].cpu().numpy()
        assert sums.dtype == np.float64 and counts.dtype == np.int64 and counts.shape == (len(thresholds),)
        print(n, len(thresholds), sums, want_sums, counts)
        assert np.array_equal(counts, want_counts)
        # both add <= ~7e4 non-negative float64 terms, in different orders: they differ by at most n 2^-53 relative (~1e-11)
        assert np.all(np.abs(sums - want_sums) <= 1e-10 * want_sums)
        assert np.array_equal(got[1][0].cpu().numpy().view(np.uint64), sums.view(np.uint64))
        assert np.array_equal(got[1][1].cpu().numpy(), counts)
        if n == 0:
            assert np.all(sums == 0) and np.all(counts == 0)
    # the host length alone (no device counter): the same numbers
    s2, c2 = hipops.recon_stats(d2[:n], ths)
    assert np.array_equal(s2.cpu().numpy().view(np.uint64), hipops.recon_stats(d2, ths, n_dev=_count(n))[0].cpu().numpy().view(np.uint64))
    assert np.array_equal(c2.cpu().numpy(), rm.stats_reference(v[:n], ths)[1])


def test_recon_stats_takes_one_to_eight_thresholds(hip):
    from nextbestpath_amd.utility import hipops
    d2 = _dev(np.array([0.0, 0.5, 2.0, 9.0], f32))
    assert hipops.recon_stats(d2, [1.0])[1].tolist() == [2]
    assert hipops.recon_stats(d2, [0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4])[1].tolist() == [1, 2, 3, 3, 3, 3, 4, 4]
    with pytest.raises(ValueError):
        hipops.recon_stats(d2, [0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5])
    with pytest.raises(ValueError):
        hipops.recon_stats(d2, [])
    with pytest.raises(ValueError):
        hipops.ReconMetrics(torch.zeros(3, 3, device="cuda"), ([0, 0, 0], [0, 0, 0]), thresholds=(6.0,), cap=5.0)    # above the cap


# ---- the metrics object
def _plane_and_cloud():
    rng = np.random.default_rng(41)
    gt = np.stack([rng.uniform(0, 30, 2000), np.full(2000, 2.0), rng.uniform(0, 20, 2000)], 1).astype(f32)
    near = np.stack([rng.uniform(-1, 31, 4200), 2.0 + rng.normal(0, 0.4, 4200), rng.uniform(-1, 21, 4200)], 1).astype(f32)
    outl = rng.uniform([-8, -8, -8], [38, 12, 28], (800, 3)).astype(f32)       # some inside the grown box, some beyond it
    cloud = np.concatenate([near, outl])
    rng.shuffle(cloud)
    return gt, cloud


def _assert_block_equals(got, want):
    assert set(got) == set(want)
    for key in ("n_points", "n_gt", "cap"):
        assert got[key] == want[key], key
    for key in ("accuracy_mean", "accuracy_rmse", "completeness_mean", "completeness_rmse", "chamfer"):
        assert abs(got[key] - want[key]) <= 1e-10 * abs(want[key]), (key, got[key], want[key])
    assert len(got["thresholds"]) == len(want["thresholds"])
    for g, w in zip(got["thresholds"], want["thresholds"]):
        assert g == w, (g, w)                      # ratios of equal integer counts: equal floats


def test_recon_metrics_summary_equals_the_numpy_reference(hip):
    from nextbestpath_amd.utility import hipops
    gt, cloud = _plane_and_cloud()
    ths = (0.5, 1.0, 2.0)
    want = rm.reference(cloud, gt, ths, cap=5.0)
    assert 0.05 < want["thresholds"][1]["precision"] < 0.95 and want["accuracy_mean"] > 0.3
    gtd = _dev(gt)
    buf = torch.full((6000, 3), float("nan"), device="cuda")                    # a rollout's buffer: capacity beyond the count
    buf[:len(cloud)] = _dev(cloud)
    buf[len(cloud):len(cloud) + 500] = gtd[:500]                                # ... with would-be perfect points in the tail
    m = hipops.ReconMetrics(gtd, (gt.min(0).tolist(), gt.max(0).tolist()), ths, cap=5.0)
    res = m.evaluate(buf, _count(len(cloud)))
    assert res["acc_sums"].dtype == torch.float64 and res["comp_counts"].dtype == torch.int64 and res["acc_sums"].is_cuda
    got = m.summary()
    print(got, want)
    _assert_block_equals(got, want)
    json.dumps(got, allow_nan=False)
    first = m.raw()
    m.evaluate(buf, _count(len(cloud)))
    assert np.array_equal(m.raw().view(np.uint64), first.view(np.uint64))       # two evaluations: the same bits
    # an empty cloud: every GT point at the cap, no NaN
    m.evaluate(buf, _count(0))
    empty = m.summary()
    assert empty == rm.reference(cloud[:0], gt, ths, cap=5.0)
    json.dumps(empty, allow_nan=False)
    # the host length alone
    m.evaluate(_dev(cloud))
    _assert_block_equals(m.summary(), want)


def test_recall_count_at_the_coverage_radius_is_the_coverage_count(hip):
    """With N <= 2 G the coverage metric does not sub-sample: its count of GT points with a cloud point closer than 1.0 is the
    recall count at threshold 1.0 (the same fp32 expression, the same `<`)."""
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(43)
    G, N = 1500, 2600
    gt = np.stack([rng.uniform(0, 40, G), rng.uniform(0, 3, G), rng.uniform(0, 40, G)], 1).astype(f32)
    cloud = np.concatenate([gt[rng.integers(0, G // 2, N - 400)] + rng.normal(0, 0.6, (N - 400, 3)),
                            rng.uniform(-10, 50, (400, 3))]).astype(f32)
    gtd, cd = _dev(gt), _dev(cloud)
    bbox = (gt.min(0).tolist(), gt.max(0).tolist())
    cov = hipops.coverage_count(gtd, cd, threshold=1.0, bbox=bbox).cpu().numpy()
    assert cov[1] == N                                                          # every point was used
    m = hipops.ReconMetrics(gtd, bbox, thresholds=(1.0,), cap=5.0)
    res = m.evaluate(cd)
    recall_count = int(res["comp_counts"][0])
    assert recall_count == int(cov[0]) and 0 < recall_count < G
    plan_out = torch.zeros(2, dtype=torch.int32, device="cuda")
    hipops.CoveragePlan(gtd, 1.0, 2, bbox).count(cd, plan_out)
    assert int(plan_out[0]) == recall_count


# ---- the driver
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=i, cells=8, size=4.8, height=1.2, tess=0.3)
    return str(d)


def _net():
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    return net.cuda().eval()


def _small_params():
    """The default parameters with a thinner GT surface and a thinner cloud, so that the numpy brute force over the rollout's whole
    cloud takes seconds (3 k GT points x ~40 k cloud points)."""
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    params.n_gt_surface_points = 3000
    params.gathering_factor = 0.005
    return params


@pytest.fixture(scope="module")
def rollout_on(hip, dataset, nbp_weights):
    """The 12-pose rollout with the option on -> (result, cloud, gt, options)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, ds, net = _small_params(), sc.SceneDataset(dataset), _net()
    opts = {"thresholds": [0.5, 1.0], "cap": 4.0}
    with torch.no_grad():
        ro = tp.build_rollout(params, net, ds, tp.list_runs(ds, params)[0], torch.device("cuda"), seed=5, recon_metrics=opts)
        for _ in range(12):
            ro.step()
        ro.finish()
        res = tp._result(ro, 12)
    n = int(ro.st.cloud_count.item())
    return res, ro.st.cloud[:n].cpu().numpy(), ro.gt.cpu().numpy(), opts


def test_rollout_reports_the_reference_metrics_of_its_cloud(rollout_on):
    res, cloud, gt, opts = rollout_on
    block = res["reconstruction"]
    assert block["n_points"] == res["n_points"] == len(cloud) > 1000 and block["n_gt"] == len(gt)
    want = rm.reference(cloud, gt, opts["thresholds"], opts["cap"])
    print(block, want)
    _assert_block_equals(block, want)
    assert [r["threshold"] for r in block["thresholds"]] == [0.5, 1.0]
    # the coverage curve looks at a sub-sample of an earlier cloud: the whole final cloud recalls at least as much
    assert block["thresholds"][1]["recall"] >= res["coverage"][-1] > 0
    assert rm.summarise_raw(res["reconstruction_raw"], opts["thresholds"], opts["cap"]) == block
    json.dumps(res["reconstruction"], allow_nan=False)


def test_rollout_with_the_option_off_is_what_it_was(hip, dataset, nbp_weights, monkeypatch):
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import hipops
    params, ds, net = _small_params(), sc.SceneDataset(dataset), _net()
    built = []
    real = hipops.ReconMetrics
    monkeypatch.setattr(hipops, "ReconMetrics", lambda *a, **k: built.append(1) or real(*a, **k))
    with torch.no_grad():
        res = tp.run_one(params, net, ds, tp.list_runs(ds, params)[0], torch.device("cuda"), n_poses=3, seed=5)
        assert not built                                                        # nothing new is constructed
        assert sorted(res) == ["V_cam_history", "X_cam_history", "coverage", "n_points", "scene", "start"]
        res["run_id"] = 0
        assert pr.pack_results([res], [(0, 0)], 3, 1).shape == (1, 3 + 3)       # the gathered row: n_poses + 3
        gathered = pr.gather_results([res], [(0, 0)], 0, 1, torch.device("cuda"), 3)
        assert "reconstruction" not in gathered[0]
        # the public method works on a rollout built without the option, and leaves its results as they were
        ro = tp.build_rollout(params, net, ds, tp.list_runs(ds, params)[0], torch.device("cuda"), seed=5)
        for _ in range(2):
            ro.step()
        block = ro.reconstruction_metrics()
        assert built and block["cap"] == 5.0 and [r["threshold"] for r in block["thresholds"]] == [1.0] and block["n_points"] > 0
        assert "reconstruction" not in tp._result(ro, 2)
        on = tp.run_one(params, net, ds, tp.list_runs(ds, params)[0], torch.device("cuda"), n_poses=3, seed=5, recon_metrics=True)
    assert on["coverage"] == res["coverage"] and on["X_cam_history"] == res["X_cam_history"]      # the option moves nothing else
    on["run_id"] = 0
    got = pr.gather_reconstruction([on], [(0, 0)], 0, 1, torch.device("cuda"), (1.0,), 5.0)
    assert got == {0: on["reconstruction"]}


def test_entry_point_json_carries_the_reconstruction_block(hip, dataset):
    cfg = {"numGPU": 0, "dataset_path": dataset, "test_scenes": [], "params_name":
           "macarons_default_training_config.json", "model_name": "x.pth", "results_json_name": "out_test_recon.json",
           "test_resolution": 0.05, "use_perfect_depth_map": True, "compute_collision": False, "load_json": False,
           "random_seed": 8, "torch_seed": 9, "nbp_weights": "./weights/none.pth",
           "recon_metrics": {"thresholds": [1.0, 2.0], "cap": 5.0}}
    cfg_path = os.path.join(ROOT, "configs/test/_pytest_recon.json")
    out_path = os.path.join(ROOT, "data", "out_test_recon.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "test_nbp_planning.py"), "-c", "_pytest_recon.json", "--n-poses", "3"],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        with open(out_path) as fh:
            text = fh.read()
        assert "NaN" not in text
        out = json.loads(text)
        assert sorted(out) == ["maze_00", "maze_01"]
        for scene in out.values():
            for rec in scene.values():
                assert set(rec) >= {"coverage", "auc", "reconstruction"} and len(rec["coverage"]) == 3
                block = rec["reconstruction"]
                assert set(block) == {"n_points", "n_gt", "cap", "accuracy_mean", "accuracy_rmse", "completeness_mean",
                                      "completeness_rmse", "chamfer", "thresholds"}
                assert block["n_points"] > 1000 and block["cap"] == 5.0 and 0 < block["accuracy_mean"] <= 5.0
                assert [t["threshold"] for t in block["thresholds"]] == [1.0, 2.0]
                assert block["thresholds"][0]["recall"] >= rec["coverage"][-1]
                assert block["thresholds"][1]["recall"] >= block["thresholds"][0]["recall"]
    finally:
        os.remove(cfg_path)
        if os.path.exists(out_path):
            os.remove(out_path)
