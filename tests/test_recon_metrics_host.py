"""The definition of the reconstruction-quality metrics (utility/recon_metrics.py, numpy): closed-form cases, the ratios formed
from hand-made sums and counts, and the squared-distance form of the threshold decision."""
import json
import math

import numpy as np
import pytest

from nextbestpath_amd.utility import recon_metrics as rm


def _lattice(n=12, step=0.5):
    a = np.arange(n, dtype=np.float32) * np.float32(step)
    x, z = np.meshgrid(a, a, indexing="ij")
    return np.stack([x.ravel(), np.zeros(n * n, np.float32), z.ravel()], 1)


def test_shifted_plane_lattice_gives_the_shift():
    gt = _lattice()
    d = 0.25                                        # exact in fp32, below half the lattice step: the nearest point is the twin
    cloud = gt + np.array([0, d, 0], np.float32)
    m = rm.reference(cloud, gt, thresholds=(0.125, 1.0), cap=5.0)
    assert m["n_points"] == m["n_gt"] == len(gt) and m["cap"] == 5.0
    for key in ("accuracy_mean", "accuracy_rmse", "completeness_mean", "completeness_rmse", "chamfer"):
        assert m[key] == pytest.approx(d, abs=1e-12), key
    below, above = m["thresholds"]
    assert (below["precision"], below["recall"], below["fscore"]) == (0.0, 0.0, 0.0)          # d is not < 0.125
    assert (above["precision"], above["recall"], above["fscore"]) == (1.0, 1.0, 1.0)
    assert [r["threshold"] for r in m["thresholds"]] == [0.125, 1.0]


def test_far_outliers_cost_precision_and_sit_at_the_cap():
    gt = _lattice()
    n_out = len(gt) // 4                            # share 0.2 of the cloud
    rng = np.random.default_rng(3)
    far = rng.uniform(-1, 1, (n_out, 3)).astype(np.float32) + np.array([0, 40, 0], np.float32)   # 39+ from the plane: beyond cap
    inside_box_but_far = np.array([[2.0, 4.5, 2.0]], np.float32)                                 # in the grown box, 4.5 away
    cloud = np.concatenate([gt + np.array([0, 0.25, 0], np.float32), far])
    m = rm.reference(cloud, gt, thresholds=(1.0,), cap=5.0)
    share = n_out / len(cloud)
    assert m["thresholds"][0]["precision"] == pytest.approx(1 - share, abs=1e-15)
    assert m["thresholds"][0]["recall"] == 1.0
    assert m["accuracy_mean"] == pytest.approx((1 - share) * 0.25 + share * 5.0, abs=1e-12)
    assert m["accuracy_rmse"] == pytest.approx(math.sqrt((1 - share) * 0.25 ** 2 + share * 25.0), abs=1e-12)
    assert m["completeness_mean"] == pytest.approx(0.25, abs=1e-12)                              # outliers do not touch it
    m2 = rm.reference(np.concatenate([cloud, inside_box_but_far]), gt, thresholds=(1.0,), cap=5.0)
    assert m2["accuracy_mean"] == pytest.approx((m["accuracy_mean"] * len(cloud) + 4.5) / (len(cloud) + 1), abs=1e-12)


def test_empty_cloud_has_no_nan():
    gt = _lattice(5)
    m = rm.reference(np.zeros((0, 3), np.float32), gt, thresholds=(1.0, 2.0), cap=3.0)
    assert m["n_points"] == 0 and m["n_gt"] == 25
    assert m["accuracy_mean"] is None and m["accuracy_rmse"] is None and m["chamfer"] is None
    assert m["completeness_mean"] == 3.0 and m["completeness_rmse"] == 3.0                       # every GT point at the cap
    for row in m["thresholds"]:
        assert row["precision"] is None and row["recall"] == 0.0 and row["fscore"] is None
    text = json.dumps(m, allow_nan=False)                                                        # raises on a NaN
    assert "NaN" not in text


def test_summarise_from_hand_made_counts():
    m = rm.summarise(acc_sums=[30.0, 160.0], acc_counts=[6, 8], n_rec=10, comp_sums=[8.0, 36.0], comp_counts=[1, 2], n_gt=4,
                     thresholds=(0.5, 1.0), cap=5.0)
    assert m["accuracy_mean"] == 3.0 and m["accuracy_rmse"] == 4.0
    assert m["completeness_mean"] == 2.0 and m["completeness_rmse"] == 3.0
    assert m["chamfer"] == 2.5
    a, b = m["thresholds"]
    assert (a["precision"], a["recall"]) == (0.6, 0.25) and a["fscore"] == pytest.approx(2 * 0.6 * 0.25 / 0.85, abs=1e-15)
    assert (b["precision"], b["recall"]) == (0.8, 0.5) and b["fscore"] == pytest.approx(2 * 0.8 * 0.5 / 1.3, abs=1e-15)
    zero = rm.summarise([5.0, 25.0], [0], 1, [5.0, 25.0], [0], 1, (1.0,), 5.0)["thresholds"][0]
    assert zero == {"threshold": 1.0, "precision": 0.0, "recall": 0.0, "fscore": 0.0}            # 0 / 0 is 0, not NaN
    raw = rm.pack_raw([30.0, 160.0], [6, 8], 10, [8.0, 36.0], [1, 2], 4)
    assert raw.dtype == np.float64 and raw.shape == (rm.RAW_HEAD + 4,)
    assert rm.summarise_raw(raw, (0.5, 1.0), 5.0) == m
    with pytest.raises(ValueError):
        rm.summarise_raw(raw, (1.0,), 5.0)


@pytest.mark.parametrize("thr", [1.0, 0.5, 0.3, 0.1, 2.5, 1.0 / 3.0, 4.999, 1e-3, 123.456])
def test_squared_threshold_decision_is_the_fp32_sqrt_decision(thr):
    t = np.float32(thr)
    bound = rm.sq_below(t)
    assert bound.dtype == np.float32
    v = np.float32(t * t)
    around = [v]
    lo = hi = v
    for _ in range(40):                                       # 40 floats on either side of t^2
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
        around += [lo, hi]
    around = np.array(around + [0.0, bound, np.nextafter(bound, np.float32(np.inf))], np.float32)
    by_root = np.sqrt(around) < t
    assert np.sqrt(around).dtype == np.float32
    assert np.array_equal(around <= bound, by_root)
    assert by_root.any() and not by_root.all()                # the values straddle the decision
    sums, counts = rm.stats_reference(around, [t])
    assert counts[0] == np.count_nonzero(around <= bound)


def test_options_are_checked():
    assert rm.option_spec(None) is None and rm.option_spec(False) is None
    assert rm.option_spec(True) == {"thresholds": (1.0,), "cap": 5.0, "cell": 1.0}
    assert rm.option_spec({"thresholds": [0.5, 1], "cap": 3}) == {"thresholds": (0.5, 1.0), "cap": 3.0, "cell": 1.0}
    for bad in ({"thresholds": [6.0]}, {"thresholds": []}, {"thresholds": list(range(1, 10)), "cap": 20.0}, {"cap": 0.0},
                {"cell": -1.0}, {"radius": 1.0}, "on", {"thresholds": [float("nan")]}):
        with pytest.raises(ValueError):
            rm.option_spec(bad)


def test_brute_force_ignores_targets_outside_the_box_and_chunks():
    rng = np.random.default_rng(5)
    q = rng.uniform(-3, 3, (50, 3)).astype(np.float32)
    t = rng.uniform(-3, 3, (70, 3)).astype(np.float32)
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    a = rm.nn_dist2_reference(q, t, lo, hi, 2.0)
    b = rm.nn_dist2_reference(q, t, lo, hi, 2.0, chunk=64)
    inside = t[np.all((t >= lo) & (t <= hi), 1)]
    want = np.minimum(((inside[None].astype(np.float64) - q[:, None]) ** 2).sum(-1).min(1), 4.0)
    assert np.array_equal(a, b) and a.dtype == np.float32
    assert np.allclose(a, want, rtol=1e-6, atol=0)
    tn = np.concatenate([t, np.full((1, 3), np.nan, np.float32)])
    assert np.array_equal(rm.nn_dist2_reference(q, tn, lo, hi, 2.0), a)
    assert np.array_equal(rm.nn_dist2_reference(q, t[:0], lo, hi, 2.0), np.full(50, 4.0, np.float32))


# ---- the second gather (CPU, gloo): raw float64 sums and counts travel, rank 0 forms the ratios
def _raw_of(rid):
    return rm.pack_raw([10.0 + rid + 1e-9, 50.0 + rid], [3 + rid, 5 + rid], 10 + rid, [2.0, 3.0 + rid], [1, 2 + rid], 4 + rid)


def _gather_worker(rank, world, port, n_runs, q):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    runs = [(i, 0) for i in range(n_runs)]
    results = [{"run_id": runs.index(run), "reconstruction_raw": _raw_of(runs.index(run)).tolist()} for run in pr.shard(runs, r, w)]
    out = pr.gather_reconstruction(results, runs, r, w, torch.device("cpu"), (0.5, 1.0), 5.0)
    q.put((r, out))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gather_reconstruction_world2_and_single_process():
    import socket

    import torch
    import torch.multiprocessing as mp
    from nextbestpath_amd import parallel_rollout as pr
    n_runs, world = 3, 2                             # odd count: rank 1 has a padded row
    want = {rid: rm.summarise_raw(_raw_of(rid), (0.5, 1.0), 5.0) for rid in range(n_runs)}
    assert want[1]["accuracy_mean"] == (11.0 + 1e-9) / 11                      # float64 all the way: fp32 would lose the 1e-9
    single = pr.gather_reconstruction([{"run_id": i, "reconstruction_raw": _raw_of(i).tolist()} for i in range(n_runs)],
                                      [(i, 0) for i in range(n_runs)], 0, 1, torch.device("cpu"), (0.5, 1.0), 5.0)
    assert single == want
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, n_runs, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0] == want and got[1] == {}           # the ratios are formed on rank 0
