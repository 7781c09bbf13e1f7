"""The numpy definition of the planner-facing validation metrics (nextbestpath_amd/utility/metrics.py) against a plain-Python
restatement written here (loops over samples, thresholds, pixels and pairs; no helper shared with the module), one case computed by
hand, the edge semantics one by one, and `summarize`."""
import json
import math

import numpy as np
import pytest

from nextbestpath_amd.utility import metrics as M


# ---- the restatement: Python floats (float32 values are exact doubles, so comparisons agree with fp32's)
def _restate(out1, out2, gt, coords, gains, bidx, thresholds):
    B, V, S = out1.shape[0], out1.shape[-1], out2.shape[-1]
    obst = [[[0, 0, 0, 0] for _ in thresholds] for _ in range(B)]
    rank = [[0] * 6 for _ in range(B)]
    val = [[0.0] * 4 for _ in range(B)]
    for b in range(B):
        for t, tau in enumerate(thresholds):
            tau32 = float(np.float32(tau))
            for r in range(S):
                for c in range(S):
                    v, lab = float(out2[b, 0, r, c]), float(gt[b, 0, r, c]) > 0.5
                    pos = (not math.isnan(v)) and v >= tau32
                    obst[b][t][(0 if lab else 1) if pos else (2 if lab else 3)] += 1
        ps, gs = [], []
        for k in range(len(bidx)):
            if int(bidx[k]) != b:
                continue
            h, r, c = (int(x) for x in coords[k])
            if not (0 <= h < 8 and 0 <= r < V and 0 <= c < V):
                rank[b][1] += 1
                continue
            ps.append(float(out1[b, h, r, c]))
            gs.append(float(gains[k]))
        n = rank[b][0] = len(ps)
        if n == 0:
            continue
        for i in range(n):
            for j in range(i + 1, n):
                if gs[i] == gs[j]:
                    continue
                rank[b][2] += 1
                if math.isnan(ps[i]) or math.isnan(ps[j]) or ps[i] == ps[j]:
                    continue
                if (ps[i] > ps[j]) == (gs[i] > gs[j]):
                    rank[b][3] += 1
                else:
                    rank[b][4] += 1
        best = None
        for i in range(n):
            if not math.isnan(ps[i]) and (best is None or ps[i] > ps[best]):
                best = i
        if best is None:
            best = 0
        rank[b][5] = int(gs[best] == max(gs))
        val[b] = [math.fsum(abs(p - g) for p, g in zip(ps, gs)), math.fsum((p - g) ** 2 for p, g in zip(ps, gs)), max(gs), gs[best]]
    return np.array(obst, np.int64).reshape(B, len(thresholds), 4), np.array(rank, np.int64), np.array(val, np.float64)


def _case(rng, B, S, counts, bad=0, nan1=0, nan2=0, shuffle=True):
    V = S // 4
    out1 = rng.choice(np.linspace(-1, 3, 9), size=(B, 8, V, V)).astype(np.float32)          # few distinct values: ties in p
    out2 = rng.random((B, 1, S, S)).astype(np.float32)
    gt = (rng.random((B, 1, S, S)) < 0.3).astype(np.float32)
    K = int(sum(counts))
    bidx = np.repeat(np.arange(B), counts).astype(np.int64)
    coords = np.stack([rng.integers(0, 8, K), rng.integers(0, V, K), rng.integers(0, V, K)], 1).astype(np.int64)
    d = rng.integers(-2, 4, K)
    gains = np.where(d > 0, d * 100, 0).astype(np.float32)                                   # ties and zeros, as real records
    if K > 1:
        coords[K // 2] = coords[0]                                                           # a duplicate cell
    for k in rng.choice(K, size=min(bad, K), replace=False):
        coords[k, rng.integers(0, 3)] = rng.choice([-1, 8 if rng.random() < 0.5 else V, 2 ** 40])
    for _ in range(nan1):
        out1[rng.integers(0, B), rng.integers(0, 8), rng.integers(0, V), rng.integers(0, V)] = np.nan
    for _ in range(nan2):
        out2[rng.integers(0, B), 0, rng.integers(0, S), rng.integers(0, S)] = np.nan
    if shuffle:
        perm = rng.permutation(K)
        coords, gains, bidx = coords[perm], gains[perm], bidx[perm]
    return out1, out2, gt, coords, gains, bidx


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:, 2:], b[2][:, 2:])
            and np.allclose(a[2][:, :2], b[2][:, :2], rtol=1e-12, atol=0, equal_nan=True))


@pytest.mark.parametrize("seed,B,S,counts,bad,nan1,nan2", [
    (1, 1, 8, [5], 0, 0, 0),
    (2, 3, 8, [0, 1, 9], 0, 0, 0),
    (3, 2, 12, [17, 2], 3, 0, 0),
    (4, 3, 8, [6, 0, 12], 2, 40, 30),
    (5, 2, 8, [30, 30], 4, 200, 10),
])
def test_definition_matches_the_plain_python_restatement(seed, B, S, counts, bad, nan1, nan2):
    rng = np.random.default_rng(seed)
    case = _case(rng, B, S, counts, bad, nan1, nan2)
    ts = (0.13, 0.0, 1.0, float(case[1][0, 0, 1, 1]))[:1 + seed % 4]
    got = M.validation_metrics_reference(*case, ts)
    want = _restate(*case, ts)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert got[0].shape == (B, len(ts), 4) and got[1].shape == (B, 6) and got[2].shape == (B, 4)
    assert _same(got, want), (got, want)
    assert np.all(got[0].sum(axis=2) == S * S)


def _hand_case():
    out1 = np.zeros((2, 8, 4, 4), np.float32)
    out1[0, 1, 2, 3], out1[0, 0, 0, 0], out1[1, 7, 3, 3] = 0.5, 2.0, -1.0
    out2 = np.zeros((2, 1, 16, 16), np.float32)
    gt = np.zeros((2, 1, 16, 16), np.float32)
    out2[0, 0, 0, :4] = [np.float32(0.13), 0.2, 0.6, 0.1]
    gt[0, 0, 0, :4] = [1, 0, 1, 1]
    gt[0, 0, 5, 5] = 1
    out2[1] = 0.9
    gt[1, 0, 15, 15] = 1
    coords = np.array([[1, 2, 3], [7, 3, 3], [1, 2, 3], [0, 0, 0]], np.int64)       # targets 0 and 2: one cell, two gains
    gains = np.array([1.0, 3.0, 2.0, 2.0], np.float32)                              # targets 2 and 3: a tie in g
    bidx = np.array([0, 1, 0, 0], np.int64)
    return out1, out2, gt, coords, gains, bidx


def test_hand_computed_case():
    obst, rank, val = M.validation_metrics_reference(*_hand_case(), (0.13, 0.5))
    assert obst.tolist() == [[[2, 1, 2, 251], [1, 0, 3, 252]], [[1, 255, 0, 0], [1, 255, 0, 0]]]
    # sample 0: p = (.5, .5, 2), g = (1, 2, 2): pair (0,1) comparable with tied p, (0,2) concordant, (1,2) tied in g
    assert rank.tolist() == [[3, 0, 2, 1, 0, 1], [1, 0, 0, 0, 0, 1]]
    assert val.tolist() == [[2.0, 2.5, 2.0, 2.0], [4.0, 16.0, 3.0, 3.0]]
    s = M.summarize(obst, rank, val, (0.13, 0.5))
    assert (s["n_samples"], s["n_targets"], s["n_bad_targets"]) == (2, 4, 0)
    assert s["value_mae"] == 1.5 and s["value_rmse"] == math.sqrt(18.5 / 4)
    assert s["rank_accuracy"] == 0.75 and s["top1_hit_rate"] == 1.0 and s["mean_regret"] == 0.0
    o = s["obstacle"]
    assert [e["threshold"] for e in o] == [0.13, 0.5]
    assert o[0] == {"threshold": 0.13, "precision": 3 / 259, "recall": 3 / 5, "iou": 3 / 261, "f1": 6 / 264}
    assert o[1] == {"threshold": 0.5, "precision": 2 / 257, "recall": 2 / 5, "iou": 2 / 260, "f1": 4 / 262}


def _tiny(p, g, coords=None, V=2, bidx=None):
    """One sample with S = 8 whose targets sit in channel 0, row 0, columns 0.. with the values p."""
    out1 = np.zeros((1, 8, V, V), np.float32)
    n = len(g)
    if coords is None:
        coords = np.array([[k // (V * V), (k // V) % V, k % V] for k in range(n)], np.int64).reshape(-1, 3)
        for k in range(n):
            out1[0, coords[k, 0], coords[k, 1], coords[k, 2]] = p[k]
    z = np.zeros((1, 1, 4 * V, 4 * V), np.float32)
    return out1, z, z, coords, np.asarray(g, np.float32), np.zeros(n, np.int64) if bidx is None else bidx


def test_threshold_is_inclusive_and_nan_is_negative():
    out1 = np.zeros((1, 8, 2, 2), np.float32)
    out2 = np.zeros((1, 1, 8, 8), np.float32)
    gt = np.ones((1, 1, 8, 8), np.float32)
    out2[0, 0, 0, 0] = np.float32(0.13)                       # exactly the fp32 threshold: positive
    out2[0, 0, 0, 1] = np.nextafter(np.float32(0.13), np.float32(0))
    out2[0, 0, 0, 2] = np.nan
    e = np.zeros((0,), np.int64)
    obst, rank, val = M.validation_metrics_reference(out1, out2, gt, e.reshape(0, 3), e.astype(np.float32), e, [0.13])
    assert obst.tolist() == [[[1, 0, 63, 0]]]
    gt[0, 0, 0, 2] = 0
    obst, _, _ = M.validation_metrics_reference(out1, out2, gt, e.reshape(0, 3), e.astype(np.float32), e, [0.13])
    assert obst.tolist() == [[[1, 0, 62, 1]]]                 # the NaN pixel: a true negative
    assert rank.tolist() == [[0] * 6] and val.tolist() == [[0.0] * 4]          # K_b = 0


def test_nan_value_is_neither_concordant_nor_discordant_and_never_best():
    nan = float("nan")
    _, rank, val = M.validation_metrics_reference(*_tiny([nan, 1.0, 2.0], [5.0, 1.0, 2.0]), [0.13])
    assert rank.tolist() == [[3, 0, 3, 1, 0, 0]]              # pred_best = target 2 (g = 2), max g = 5: no hit
    assert val[0, 2:].tolist() == [5.0, 2.0] and np.isnan(val[0, 0]) and np.isnan(val[0, 1])
    _, rank, val = M.validation_metrics_reference(*_tiny([nan, nan], [1.0, 7.0]), [0.13])
    assert rank.tolist() == [[2, 0, 1, 0, 0, 0]] and val[0, 3] == 1.0          # every p NaN: the first good target
    _, rank, val = M.validation_metrics_reference(*_tiny([nan, -np.inf, -np.inf], [1.0, 7.0, 9.0]), [0.13])
    assert rank[0, 5] == 0 and val[0, 3] == 7.0               # -inf beats a NaN; the first of the two wins


def test_first_maximum_wins():
    _, rank, val = M.validation_metrics_reference(*_tiny([1.0, 3.0, 3.0, 2.0], [0.0, 4.0, 9.0, 9.0]), [0.13])
    # pairs: (0,1) (0,2) (0,3) concordant, (1,2) tied in p, (1,3) discordant, (2,3) tied in g; the first p = 3 is target 1
    assert rank.tolist() == [[4, 0, 5, 3, 1, 0]] and val[0, 2:].tolist() == [9.0, 4.0]


def test_bad_coordinates_are_counted_and_ignored():
    out1, z, _, coords, gains, bidx = _tiny([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])
    bad = np.array([[8, 0, 0], [0, -1, 0], [0, 0, 2], [-1, 0, 0], [0, 2 ** 40, 0]], np.int64)
    c2 = np.concatenate([bad[:2], coords[:1], bad[2:4], coords[1:], bad[4:]])
    g2 = np.concatenate([[50.0, 60.0], gains[:1], [70.0, 80.0], gains[1:], [90.0]]).astype(np.float32)
    a = M.validation_metrics_reference(out1, z, z, coords, gains, bidx, [0.13])
    b = M.validation_metrics_reference(out1, z, z, c2, g2, np.zeros(8, np.int64), [0.13])
    assert b[1].tolist() == [[3, 5, 3, 3, 0, 1]] and a[1].tolist() == [[3, 0, 3, 3, 0, 1]]
    assert np.array_equal(a[2], b[2]) and b[2].tolist() == [[0.0, 0.0, 3.0, 3.0]]
    only_bad = M.validation_metrics_reference(out1, z, z, bad, g2[:5], np.zeros(5, np.int64), [0.13])
    assert only_bad[1].tolist() == [[0, 5, 0, 0, 0, 0]] and only_bad[2].tolist() == [[0.0] * 4]


def test_single_target_and_empty_sample():
    out1, z, _, coords, gains, _ = _tiny([1.5], [4.0])
    out1 = np.concatenate([out1, out1, out1])
    z3 = np.zeros((3, 1, 8, 8), np.float32)
    _, rank, val = M.validation_metrics_reference(out1, z3, z3, coords, gains, np.array([2], np.int64), [0.13])
    assert rank.tolist() == [[0] * 6, [0] * 6, [1, 0, 0, 0, 0, 1]]
    assert val.tolist() == [[0.0] * 4, [0.0] * 4, [2.5, 6.25, 4.0, 4.0]]
    s = M.summarize(np.zeros((3, 1, 4), np.int64), rank, val, [0.13])
    assert s["rank_accuracy"] is None and s["top1_hit_rate"] == 1.0 and s["n_samples"] == 3 and s["value_mae"] == 2.5


def test_unsorted_bidx_gives_the_sorted_result():
    rng = np.random.default_rng(11)
    out1, out2, gt, coords, gains, bidx = _case(rng, 3, 8, [7, 0, 11], bad=2, shuffle=False)
    a = M.validation_metrics_reference(out1, out2, gt, coords, gains, bidx, [0.13])
    # a shuffle that keeps every sample's own order (record order is part of the definition: it breaks ties of p)
    key = rng.random(len(bidx))
    perm = np.array(sorted(range(len(bidx)), key=lambda k: (key[k] > 0.5, k)))
    assert not np.all(np.diff(bidx[perm]) >= 0)
    b = M.validation_metrics_reference(out1, out2, gt, coords[perm], gains[perm], bidx[perm], [0.13])
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2][:, 2:], b[2][:, 2:])
    assert np.allclose(a[2], b[2], rtol=1e-12, atol=0)
    # any shuffle at all: everything that does not depend on the order of equal p's
    perm = rng.permutation(len(bidx))
    c = M.validation_metrics_reference(out1, out2, gt, coords[perm], gains[perm], bidx[perm], [0.13])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1][:, :5], c[1][:, :5]) and np.array_equal(a[2][:, 2], c[2][:, 2])


def test_summarize_zero_denominators_are_none_and_json_survives():
    s = M.summarize(np.zeros((2, 2, 4), np.int64), np.zeros((2, 6), np.int64), np.zeros((2, 4)), (0.13, 0.5))
    assert s["n_samples"] == 2 and s["n_targets"] == 0 and s["n_bad_targets"] == 0
    for k in ("value_mae", "value_rmse", "rank_accuracy", "top1_hit_rate", "mean_regret"):
        assert s[k] is None, k
    assert len(s["obstacle"]) == 2
    for e in s["obstacle"]:
        assert set(e) == {"threshold", "precision", "recall", "iou", "f1"}
        assert all(e[k] is None for k in ("precision", "recall", "iou", "f1"))
    text = json.dumps(s, allow_nan=False)
    assert json.loads(text) == s and "null" in text
    empty = M.summarize(np.zeros((0, 1, 4), np.int64), np.zeros((0, 6), np.int64), np.zeros((0, 4)), [0.13])
    assert empty["n_samples"] == 0 and empty["value_mae"] is None
    # a sum that is not a number (a NaN prediction) is reported as null as well, never as NaN
    _, rank, val = M.validation_metrics_reference(*_tiny([float("nan"), 1.0], [1.0, 2.0]), [0.13])
    s = M.summarize(np.zeros((1, 1, 4), np.int64), rank, val, [0.13])
    assert s["value_mae"] is None and s["value_rmse"] is None and s["rank_accuracy"] == 0.5
    json.dumps(s, allow_nan=False)


def test_totals_add_over_batches():
    rng = np.random.default_rng(21)
    ts = (0.13, 0.4)
    a = _case(rng, 2, 8, [9, 4], bad=1)
    b = _case(rng, 3, 8, [0, 1, 14])
    ra, rb = M.validation_metrics_reference(*a, ts), M.validation_metrics_reference(*b, ts)
    both = tuple(np.concatenate([x, y]) for x, y in zip(a[:3], b[:3])) + (
        np.concatenate([a[3], b[3]]), np.concatenate([a[4], b[4]]), np.concatenate([a[5], b[5] + 2]))
    whole = M.summarize(*M.validation_metrics_reference(*both, ts), ts)
    tot = M.totals(*ra) + M.totals(*rb)
    assert tot.dtype == np.float64 and tot.shape == (M.totals_size(2),)
    added = M.summarize_totals(tot, ts)
    assert added["n_samples"] == 5
    for k, v in whole.items():
        if k in ("value_mae", "value_rmse", "mean_regret"):
            assert added[k] == pytest.approx(v, rel=1e-12)
        else:
            assert added[k] == v, k
    # ratios of sums, not means of ratios
    pa, pb = M.summarize(*ra, ts), M.summarize(*rb, ts)
    assert added["rank_accuracy"] != pytest.approx((pa["rank_accuracy"] + pb["rank_accuracy"]) / 2, rel=1e-9)


def test_thresholds_are_checked():
    case = _hand_case()
    for bad in ((), tuple(range(9)), "abc", [float("nan")], [True]):
        with pytest.raises(ValueError):
            M.validation_metrics_reference(*case, bad)
    assert M.check_thresholds(0.13) == (0.13,) and M.check_thresholds([0, 1]) == (0.0, 1.0)
