"""GPU: the per-step reconstruction curve (csrc/nbp_recon.hip through hipops.ReconCurve / recon_curve_update_batch and the rollout
driver's `recon_metrics` option with `curve`) against its numpy definition (utility/recon_metrics.py::CurveReference).

The running per-GT-point minimum must equal the definition BIT FOR BIT (np.array_equal) after every update, the counts exactly, the
completeness sums bit for bit those of hipops.recon_stats over it; the accuracy sums are float64 sums of n non-negative terms in
another order: within 2 n 2^-53 relative."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_curve_cases as cases  # noqa: E402
from nextbestpath_amd.utility import recon_metrics as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN = float("nan")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, order="C")).to("cuda", dtype)            # (a copy: the shared cases are read-only)


def _count(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _curve(gt, thresholds, cap, cell=1.0, n_rows=16, **kw):
    from nextbestpath_amd.utility import hipops
    return hipops.ReconCurve(_dev(gt), (gt.min(0).tolist(), gt.max(0).tolist()), thresholds, cap, cell, n_rows=n_rows, **kw)


def _buffer(chunks, spare, tail=None):
    """One NaN-filled cloud buffer holding the chunks back to back, `spare` rows beyond them (the first of them = `tail`)."""
    total = sum(len(c) for c in chunks)
    buf = torch.full((total + spare, 3), NAN, device="cuda")
    if total:
        buf[:total] = _dev(np.concatenate(chunks))
    if tail is not None:
        buf[total:total + len(tail)] = _dev(tail)
    return buf


def _assert_acc_sums(got, want, n):
    for g, w in zip(got, want):
        assert abs(g - w) <= 2 * n * 2.0 ** -53 * abs(w), (got, want, n)


# ---- 1. the shared chunk sequence
def test_chunk_sequence_equals_the_definition(hip):
    from nextbestpath_amd.utility import hipops
    gt, chunks = cases.plane_case()
    states = cases.plane_states()
    T = len(cases.THRESHOLDS)
    buf = _buffer(chunks, 700, tail=gt[:500])                    # beyond the count: later chunks, then would-be perfect points
    cv = _curve(gt, cases.THRESHOLDS, cases.CAP, n_rows=len(chunks))
    n_dev, n, rows = _count(0), 0, []
    for k, c in enumerate(chunks):
        n += len(c)
        n_dev.fill_(n)
        bound = 1000 if len(c) == 12000 else len(c)              # 12000 new points on a grid sized for 1000: twelve passes
        row = cv.update(buf, n_dev, k, bound).cpu().numpy()
        rows.append(row)
        want_row, d2_gt, acc_sums, acc_counts, n_rec = states[k]
        assert np.array_equal(cv.d2_gt.cpu().numpy(), d2_gt), k
        assert row[4] == n_rec == n and row[5] == len(gt) and int(cv.seen) == n
        assert np.array_equal(row[6:6 + T], acc_counts) and np.array_equal(row[6 + T:], want_row[6 + T:]), k
        sums, counts = hipops.recon_stats(cv.d2_gt, cases.THRESHOLDS)
        assert np.array_equal(_bits(row[2:4]), _bits(sums.cpu().numpy())) and np.array_equal(row[6 + T:], counts.cpu().numpy())
        print(k, len(c), row[0:2], acc_sums)
        _assert_acc_sums(row[0:2], acc_sums, n)
    assert np.array_equal(_bits(cv.raw(len(chunks))), _bits(np.stack(rows)))
    curve = cv.curve(len(chunks))
    assert curve["n_points"] == [int(s[4]) for s in states] and curve["accuracy_mean"][0] is None
    assert 0.05 < curve["thresholds"][1]["recall"][-1] < 0.95
    json.dumps(curve, allow_nan=False)
    # reset: the same sequence again gives the same bits
    cv.reset()
    assert int(cv.seen) == 0
    n_dev.fill_(sum(cases.SIZES))
    whole = cv.update(buf, n_dev, 0, sum(cases.SIZES)).cpu().numpy()          # ... and the whole cloud in ONE update
    assert np.array_equal(cv.d2_gt.cpu().numpy(), states[-1][1]) and np.array_equal(whole[4:], rows[-1][4:])
    assert np.array_equal(_bits(whole[2:4]), _bits(rows[-1][2:4]))
    _assert_acc_sums(whole[0:2], rows[-1][0:2], sum(cases.SIZES))


# ---- 2. edge cases: one small case each.  A case = (gt, chunks, thresholds, cap, cell)
def _cells_1_to_5():
    """GT cells holding 1, 2, 3, 4 and 5 points (the walk takes a run four points at a time): cell centres 3 cells apart."""
    rng = np.random.default_rng(21)
    gt = np.concatenate([np.array([1.5 + 3 * k, 0.5, 0.5], f32) + rng.uniform(-0.3, 0.3, (k + 1, 3)).astype(f32) for k in range(5)])
    gt = np.concatenate([gt, [[0, 0, 0], [15, 1, 1]]]).astype(f32)               # (the box's corners)
    return gt, [rng.uniform([-1, -1, -1], [16, 2, 2], (300, 3)).astype(f32)], (0.5, 1.0), 2.0, 1.0


def _duplicates_and_exact():
    rng = np.random.default_rng(22)
    gt = rng.uniform(0, 6, (40, 3)).astype(f32)
    gt[7] = gt[3]
    new = rng.uniform(0, 6, (25, 3)).astype(f32)
    new[4] = gt[11]                                                             # exactly on a GT point
    new[5] = gt[3] + f32(0.01)
    return gt, [new], (1.0,), 3.0, 1.0


def _outside_the_grown_box():
    """GT in [0, 10]^3, cap 2: the grown box ends at 12.  New points on its face, and beyond it by less than, exactly and more than
    cap -- with and without a NaN row among them."""
    rng = np.random.default_rng(23)
    gt = rng.uniform(0, 10, (200, 3)).astype(f32)
    gt[0], gt[1] = [0, 0, 0], [10, 10, 10]
    xs = [12.0, np.nextafter(f32(12), f32(13)), 13.0, 14.0, np.nextafter(f32(14), f32(15)), 15.0, 40.0, -2.0, -3.5, -4.0, -4.5, 1e30]
    new = np.array([[x, 5.0, 5.0] for x in xs] + [[10.0, 10.0, x] for x in xs] + [[NAN, 5, 5], [5, NAN, 5], [5, 5, NAN]], f32)
    inside = rng.uniform(9, 12, (60, 3)).astype(f32)
    return gt, [np.concatenate([new, inside]), np.concatenate([inside[:9], new])], (1.0, 2.0), 2.0, 1.0


def _farther_then_nearer():
    gt = np.array([[0, 0, 0], [4, 0, 0], [8, 0, 0]], f32)
    at = lambda d: (gt + np.array([0, d, 0], f32)).astype(f32)                  # noqa: E731
    return gt, [at(1.0), at(2.0), at(0.5), at(3.0)], (0.75, 1.5), 4.0, 1.0


def _cap_over_cell(cap, cell):
    def make():
        rng = np.random.default_rng(int(cap * 10))
        gt = rng.uniform([0, 0, 0], [9, 3, 7], (400, 3)).astype(f32)
        chunks = [rng.uniform([-4, -4, -4], [13, 7, 11], (n, 3)).astype(f32) for n in (33, 150)]
        return gt, chunks, (cell, cap), cap, cell
    return make


def _eight_thresholds():
    rng = np.random.default_rng(26)
    gt = rng.uniform(0, 8, (300, 3)).astype(f32)
    return (gt, [rng.uniform(-2, 10, (n, 3)).astype(f32) for n in (50, 0, 70)], (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0), 4.0, 1.0)


EDGE_CASES = {"cells_1_to_5": _cells_1_to_5, "duplicates_and_exact": _duplicates_and_exact, "outside_box": _outside_the_grown_box,
              "farther_then_nearer": _farther_then_nearer, "cap_over_cell_2.5": _cap_over_cell(2.5, 1.0),
              "cap_over_cell_6": _cap_over_cell(3.0, 0.5), "eight_thresholds": _eight_thresholds}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_case_equals_the_definition(hip, name):
    gt, chunks, ths, cap, cell = EDGE_CASES[name]()
    T = len(ths)
    ref = rm.CurveReference(gt, ths, cap)
    cv = _curve(gt, ths, cap, cell, n_rows=len(chunks))
    buf = _buffer(chunks, 40, tail=gt[:40])
    n_dev, n, prev = _count(0), 0, np.zeros(T)
    for k, c in enumerate(chunks):
        n += len(c)
        n_dev.fill_(n)
        row = cv.update(buf, n_dev, k, len(c)).cpu().numpy()
        before = ref.acc_counts.copy()
        want = ref.update(c)
        assert np.array_equal(cv.d2_gt.cpu().numpy(), ref.d2_gt), (name, k)
        assert np.array_equal(row[6:6 + T] - prev, ref.acc_counts - before), (name, k)      # the step's own accuracy counts
        assert np.array_equal(row[4:], want[4:]), (name, k)
        _assert_acc_sums(row[0:2], want[0:2], max(n, 1))
        prev = row[6:6 + T]
    d2 = cv.d2_gt.cpu().numpy()
    if name == "duplicates_and_exact":
        assert d2[3] == d2[7] < f32(cap) ** 2 and d2[11] == 0.0                  # both duplicates are lowered; d2 = 0 on the point
    if name == "farther_then_nearer":
        assert d2.tolist() == [0.25] * 3                                         # 1.0, not raised by 2.0, lowered by 0.5, kept at 3.0
        assert cv.raw(4)[:, 2].tolist() == [3.0, 3.0, 1.5, 1.5]
    if name == "outside_box":
        assert (ref.d2_gt < f32(cap) ** 2).any() and (ref.d2_gt == f32(cap) ** 2).any()


def test_counts_capacity_nothing_new_and_the_empty_cloud(hip):
    rng = np.random.default_rng(27)
    gt = rng.uniform(0, 8, (120, 3)).astype(f32)
    pts = rng.uniform(-1, 9, (50, 3)).astype(f32)
    ths, cap = (1.0, 2.0), 3.0
    cv = _curve(gt, ths, cap, n_rows=6)
    buf, n_dev = _dev(pts), _count(0)
    ref = rm.CurveReference(gt, ths, cap)
    # the first update, on an empty cloud: every GT point at the cap, no accuracy
    row0 = cv.update(buf, n_dev, 0, 0).cpu().numpy()
    assert np.array_equal(_bits(row0), _bits(ref.update(pts[:0]))) and int(cv.seen) == 0
    assert (cv.d2_gt.cpu().numpy() == f32(cap) ** 2).all()
    first = cv.curve(1)
    assert first["accuracy_mean"] == [None] and first["chamfer"] == [None] and first["thresholds"][0]["precision"] == [None]
    assert first["completeness_mean"] == [cap] and first["thresholds"][1]["recall"] == [0.0]
    # a count beyond the capacity: the buffer's 50 rows and no more
    n_dev.fill_(80)
    row1 = cv.update(buf, n_dev, 1, 80).cpu().numpy()
    want = ref.update(pts)
    assert int(cv.seen) == 50 and row1[4] == 50 and np.array_equal(row1[4:], want[4:])
    assert np.array_equal(cv.d2_gt.cpu().numpy(), ref.d2_gt)
    # nothing new (the same count; a count that moved back): the row is repeated, the watermark and d2_gt stay
    d2 = cv.d2_gt.clone()
    for k, count in ((2, 80), (3, 50), (4, 10)):
        n_dev.fill_(count)
        again = cv.update(buf, n_dev, k, 50).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(row1)) and int(cv.seen) == 50 and torch.equal(cv.d2_gt, d2)
    assert np.array_equal(_bits(cv.raw(6)[5]), _bits(np.zeros(10)))             # a row never written stays zero


# ---- 3. batch equals singles
def _batch_setup():
    rng = np.random.default_rng(31)
    out = []
    for G, lo, hi, sizes, ths, cap in ((500, [0, 0, 0], [12, 3, 9], (40, 300, 0), (0.5, 1.0), 3.0),
                                       (1300, [-20, 5, 1], [-2, 9, 30], (0, 17, 2500), (1.0,), 5.0),
                                       (77, [3, 3, 3], [5, 4, 8], (129, 0, 64), (0.25, 0.5, 1.0, 2.0), 2.0)):
        gt = rng.uniform(lo, hi, (G, 3)).astype(f32)
        chunks = [rng.uniform(np.array(lo) - 4, np.array(hi) + 4, (n, 3)).astype(f32) for n in sizes]
        out.append((gt, chunks, ths, cap))
    return out


def _run_batch_sequence(batched):
    from nextbestpath_amd.utility import hipops
    setup = _batch_setup()
    curves = [_curve(gt, ths, cap, n_rows=3) for gt, _, ths, cap in setup]
    bufs = [_buffer(chunks, 30, tail=gt[:30]) for gt, chunks, _, _ in setup]
    counts, ns = [_count(0) for _ in setup], [0] * len(setup)
    for step in range(3):
        items = []
        for i, (gt, chunks, _, _) in enumerate(setup):
            ns[i] += len(chunks[step])
            counts[i].fill_(ns[i])
            items.append(curves[i].item(bufs[i], counts[i], step, len(chunks[step])))
        if batched:
            hipops.recon_curve_update_batch(items)
        else:
            for it in items:
                hipops.recon_curve_update_batch([it])
    return [(cv.raw(3), cv.d2_gt.cpu().numpy(), int(cv.seen)) for cv in curves]


def test_batch_equals_singles_and_repeats(hip):
    batch, singles, again = _run_batch_sequence(True), _run_batch_sequence(False), _run_batch_sequence(True)
    for i, (gt, chunks, ths, cap) in enumerate(_batch_setup()):
        ref = rm.CurveReference(gt, ths, cap)
        for c in chunks:
            ref.update(c)
        for got in (batch[i], singles[i], again[i]):
            assert np.array_equal(_bits(got[0]), _bits(batch[i][0])), i
            assert np.array_equal(got[1].view(np.uint32), batch[i][1].view(np.uint32)) and got[2] == sum(len(c) for c in chunks)
        assert np.array_equal(batch[i][1], ref.d2_gt) and np.array_equal(batch[i][0][:, 4:], np.stack(ref.rows)[:, 4:])


def test_more_items_than_one_launch_takes(hip):
    """17 curves over one GT: the call goes in chunks of 16, every curve gets its row."""
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(32)
    gt = rng.uniform(0, 5, (60, 3)).astype(f32)
    pts = rng.uniform(-1, 6, (90, 3)).astype(f32)
    buf, n_dev = _dev(pts), _count(90)
    curves = [_curve(gt, (1.0,), 2.0, n_rows=1) for _ in range(17)]
    hipops.recon_curve_update_batch([cv.item(buf, n_dev, 0, 90) for cv in curves])
    want = rm.CurveReference(gt, (1.0,), 2.0).update(pts)
    rows = [cv.raw(1)[0] for cv in curves]
    assert all(np.array_equal(_bits(r), _bits(rows[0])) for r in rows) and np.array_equal(rows[0][4:], want[4:])


# ---- 4. refusals
def test_refusals(hip):
    from nextbestpath_amd.utility import hipops
    gt = np.random.default_rng(33).uniform(0, 5, (30, 3)).astype(f32)
    gtd, bbox = _dev(gt), (gt.min(0).tolist(), gt.max(0).tolist())
    cloud, n_dev = torch.zeros(10, 3, device="cuda"), _count(10)
    with pytest.raises(RuntimeError):
        hipops.ReconCurve(torch.from_numpy(gt), bbox)                            # a CPU tensor: no CPU fallback
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd.double(), bbox)
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd.reshape(-1), bbox)
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd[:0], bbox)
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd, bbox, thresholds=(6.0,), cap=5.0)                 # a threshold above the cap
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd, ([1, 1, 1], [4, 4, 4]))                           # a box that does not hold the GT
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd, bbox, n_rows=0)
    other = hipops.ReconMetrics(_dev(gt + 1), ((gt + 1).min(0).tolist(), (gt + 1).max(0).tolist()))
    with pytest.raises(ValueError):
        hipops.ReconCurve(gtd, bbox, plan=other.plan)                            # the plan of another GT
    cv = hipops.ReconCurve(gtd, bbox, n_rows=4)
    with pytest.raises(RuntimeError):
        cv.item(cloud.cpu(), n_dev, 0, 10)
    for bad_cloud in (cloud.double(), cloud.reshape(-1), cloud[:0], torch.zeros(10, 4, device="cuda")[:, :3]):
        with pytest.raises(ValueError):
            cv.item(bad_cloud, n_dev, 0, 10)
    for bad_count in (None, n_dev.int(), n_dev.cpu(), torch.zeros(2, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            cv.item(cloud, bad_count, 0, 10)
    for bad_row in (-1, 4, 1.0, True):
        with pytest.raises(ValueError):
            cv.item(cloud, n_dev, bad_row, 10)
    with pytest.raises(ValueError):
        cv.item(cloud, n_dev, 0, -1)
    with pytest.raises(ValueError):
        cv.raw(5)
    it = cv.item(cloud, n_dev, 0, 10)
    with pytest.raises(ValueError):
        hipops.recon_curve_update_batch([it, it])                                # one curve twice in a call
    with pytest.raises(ValueError):
        hipops.recon_curve_update_batch([(cv, cloud, n_dev, 0)])
    if torch.cuda.device_count() > 1:                                            # mixed devices
        with pytest.raises(ValueError):
            cv.item(cloud.to("cuda:1"), n_dev, 0, 10)
    mixed = (cv, cloud.cpu(), n_dev, 0, 10)                                      # (an item not made by item(): the batch checks too)
    with pytest.raises(ValueError):
        hipops.recon_curve_update_batch([it, mixed])
    assert int(cv.seen) == 0 and not cv.rows.any()                               # nothing was launched


# ---- 5-8. the driver (tests/test_gpu_recon.py's small setting)
OPTS = {"thresholds": [0.5, 1.0], "cap": 4.0, "curve": True}
N_STEPS = 12


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


def _recall_covers(recall, coverage):
    """recall >= coverage, decided in the coverage's own format: coverage is fl32(count) / fl32(G) in fp32, recall count / G in
    float64.  With no sub-sampling (N <= 2 G, the first steps) the two counts are EQUAL, and the fp32 quotient may lie above the
    float64 one by its rounding; rounded to fp32 both are the correctly rounded quotient, and rounding is monotone: the comparison
    is that of the counts."""
    return np.float32(recall) >= np.float32(coverage)


def _small_params():
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    params.n_gt_surface_points = 3000
    params.gathering_factor = 0.005
    return params


def test_rollout_curve_equals_the_definition_step_by_step(hip, dataset, nbp_weights):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.lockstep import N_POSES
    from nextbestpath_amd.testers import nbp_planning as tp
    params, ds, net = _small_params(), sc.SceneDataset(dataset), _net()
    seen_counts = []
    with torch.no_grad():
        ro = tp.build_rollout(params, net, ds, tp.list_runs(ds, params)[0], torch.device("cuda"), seed=5, recon_metrics=OPTS)
        for _ in range(N_STEPS):
            seen_counts.append(int(ro.st.cloud_count.item()))
            ro.step()
        ro.finish()
        res = tp._result(ro, N_STEPS)
    n = int(ro.st.cloud_count.item())
    cloud, gt = ro.st.cloud[:n].cpu().numpy(), ro.gt.cpu().numpy()
    ths, cap, T = OPTS["thresholds"], OPTS["cap"], 2
    rows = np.asarray(res["reconstruction_curve_raw"])
    assert rows.shape == (N_STEPS, 6 + 2 * T) and seen_counts[0] == 0 < seen_counts[1] < seen_counts[-1] < n
    ref, prev = rm.CurveReference(gt, ths, cap), 0
    for s, c in enumerate(seen_counts):               # row s: the whole cloud as step s found it (what coverage[s] was counted on)
        want = ref.update(cloud[prev:c])
        prev = c
        assert np.array_equal(rows[s, 4:], want[4:]), s
        for col in range(4):
            assert abs(rows[s, col] - want[col]) <= 1e-10 * abs(want[col]), (s, col)
    curve = res["reconstruction_curve"]
    assert curve == rm.summarise_curve(rows, ths, cap) == ro.reconstruction_curve(N_STEPS)
    assert curve["n_points"] == seen_counts and curve["accuracy_mean"][0] is None
    for s in range(N_STEPS):                          # coverage looks at a sub-sample of the same cloud
        assert _recall_covers(curve["thresholds"][1]["recall"][s], res["coverage"][s]), s
    assert res["coverage"][-1] > 0
    json.dumps(curve, allow_nan=False)
    # one more update, into the spare row: the final cloud's metrics, as the whole-cloud evaluation reports them
    last = ro.recon_curve.update(ro.st.cloud, ro.st.cloud_count, N_POSES, ro.st.cloud.shape[0]).cpu().numpy()
    final = np.asarray(res["reconstruction_raw"])
    assert last[4] == final[4] == n and np.array_equal(last[4:], final[4:])
    assert np.array_equal(_bits(last[2:4]), _bits(final[2:4]))
    _assert_acc_sums(last[0:2], final[0:2], n)


def test_lockstep_gives_every_run_its_own_curve(hip, dataset, nbp_weights):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params, ds, net = _small_params(), sc.SceneDataset(dataset), _net()
    dev = torch.device("cuda")
    runs = tp.list_runs(ds, params)
    runs = [runs[0], runs[1], runs[0]]               # three runs (the first scene twice, under another seed)
    seeds = [5, 6, 7]
    with torch.no_grad():
        many = tp.run_many(params, net, ds, runs, dev, seeds, n_poses=4, rollouts_per_gpu=2, recon_metrics=OPTS)   # groups of 2 and 1
        off = tp.run_many(params, net, ds, runs, dev, seeds, n_poses=4, rollouts_per_gpu=2,
                          recon_metrics={"thresholds": [0.5, 1.0], "cap": 4.0})
        ones = [tp.run_one(params, net, ds, run, dev, n_poses=4, seed=seed, recon_metrics=OPTS) for run, seed in zip(runs, seeds)]
    for m, o, one in zip(many, off, ones):
        assert np.array_equal(_bits(m["reconstruction_curve_raw"]), _bits(one["reconstruction_curve_raw"]))
        assert m["reconstruction_curve"] == one["reconstruction_curve"] and m["reconstruction_curve"]["n_points"][-1] > 0
        assert "reconstruction_curve" not in o and "reconstruction_curve_raw" not in o
        for key in ("coverage", "X_cam_history", "V_cam_history", "n_points", "reconstruction_raw"):
            assert m[key] == o[key], key


def test_with_the_curve_off_nothing_is_built(hip, dataset, nbp_weights, monkeypatch):
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import hipops
    params, ds, net = _small_params(), sc.SceneDataset(dataset), _net()
    built, launched = [], []
    real, real_update = hipops.ReconCurve, hipops.recon_curve_update_batch
    monkeypatch.setattr(hipops, "ReconCurve", lambda *a, **k: built.append(1) or real(*a, **k))
    monkeypatch.setattr(hipops, "recon_curve_update_batch", lambda items: launched.append(len(items)) or real_update(items))
    run = tp.list_runs(ds, params)[0]
    base = ["V_cam_history", "X_cam_history", "coverage", "n_points", "scene", "start"]
    with torch.no_grad():
        for option, keys in ((None, base), (True, sorted(base + ["reconstruction", "reconstruction_raw"])),
                             ({"cap": 4.0, "curve": False}, sorted(base + ["reconstruction", "reconstruction_raw"]))):
            res = tp.run_one(params, net, ds, run, torch.device("cuda"), n_poses=3, seed=5, recon_metrics=option)
            assert not built and not launched
            assert sorted(res) == keys
            res["run_id"] = 0
            assert pr.pack_results([res], [(0, 0)], 3, 1).shape == (1, 3 + 3)
        ro = tp.build_rollout(params, net, ds, run, torch.device("cuda"), seed=5, recon_metrics=True)
        assert ro.recon_curve is None and ro.recon_curve_item() is None
        with pytest.raises(RuntimeError):
            ro.reconstruction_curve(1)
        on = tp.run_one(params, net, ds, run, torch.device("cuda"), n_poses=3, seed=5, recon_metrics={"curve": True})
    assert built == [1] and launched == [1, 1, 1]
    assert sorted(on) == sorted(base + ["reconstruction", "reconstruction_raw", "reconstruction_curve", "reconstruction_curve_raw"])
    assert on["coverage"] == res["coverage"] and on["X_cam_history"] == res["X_cam_history"]


def test_entry_point_json_carries_the_curve(hip, dataset):
    cfg = {"numGPU": 0, "dataset_path": dataset, "test_scenes": [], "params_name":
           "macarons_default_training_config.json", "model_name": "x.pth", "results_json_name": "out_test_recon_curve.json",
           "test_resolution": 0.05, "use_perfect_depth_map": True, "compute_collision": False, "load_json": False,
           "random_seed": 8, "torch_seed": 9, "nbp_weights": "./weights/none.pth",
           "recon_metrics": {"curve": True}}
    cfg_path = os.path.join(ROOT, "configs/test/_pytest_recon_curve.json")
    out_path = os.path.join(ROOT, "data", "out_test_recon_curve.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "test_nbp_planning.py"), "-c", "_pytest_recon_curve.json", "--n-poses",
                            "3"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        with open(out_path) as fh:
            text = fh.read()
        assert "NaN" not in text
        out = json.loads(text)
        assert sorted(out) == ["maze_00", "maze_01"]
        for scene in out.values():
            for rec in scene.values():
                assert set(rec) >= {"coverage", "auc", "reconstruction", "reconstruction_curve"}
                assert "reconstruction_curve_raw" not in rec and "reconstruction_raw" not in rec
                curve = rec["reconstruction_curve"]
                for key in ("n_points", "accuracy_mean", "accuracy_rmse", "completeness_mean", "completeness_rmse", "chamfer"):
                    assert len(curve[key]) == 3, key
                block = curve["thresholds"][0]
                assert block["threshold"] == 1.0 and len(block["recall"]) == len(block["precision"]) == len(block["fscore"]) == 3
                assert curve["n_points"][0] == 0 < curve["n_points"][1] < curve["n_points"][2] <= rec["reconstruction"]["n_points"]
                assert curve["accuracy_mean"][0] is None and curve["auc"]["fscore"] == [None]
                assert curve["auc"]["recall"][0] > 0
                for s in range(3):
                    assert _recall_covers(block["recall"][s], rec["coverage"][s]), s
    finally:
        os.remove(cfg_path)
        if os.path.exists(out_path):
            os.remove(out_path)
