"""Planner-facing validation metrics: the numpy definition of record (host).  csrc/nbp_metrics.hip computes the same per-sample
quantities on the device (hipops.validation_metrics); tests/test_gpu_metrics.py holds the kernel to this file.

The planner consumes the network in two ways: it thresholds out2 with `>=` (hipops.fuse_obstacle, replan_batch; 0.13) and it takes
the best-valued candidate of out1.  So, per validation sample:

  obst  int64 [B,T,4]  (tp, fp, fn, tn) of the mask `out2 >= float32(threshold)` (compared in fp32; a NaN is negative) against the
                       label `gt > 0.5`, per threshold.
  rank  int64 [B,6]    (n, n_bad, comparable, concordant, discordant, hit) over the sample's targets in record order.  A target
                       whose heading is outside [0,8) or whose row / column is outside [0,V) is bad: counted in n_bad, ignored
                       otherwise; n counts the good ones.  p_k = out1[b, heading, row, col], g_k = gains[k].  Over the pairs i < j
                       of good targets with g_i != g_j: comparable counts them all, concordant those with (p_i - p_j)(g_i - g_j) > 0,
                       discordant those with < 0 -- the sign of the exact product, i.e. decided by comparisons (p_i > p_j and
                       g_i > g_j, ...), so that neither an underflow nor inf - inf can change it; a NaN p makes neither.
                       pred_best is the first good target of maximal p; a NaN never wins; if every p is NaN it is the first good
                       target.  hit = 1 iff g[pred_best] == max g (0 when n == 0).
  val   float64 [B,4]  (sum |p - g|, sum (p - g)^2, max g, g[pred_best]) over the good targets, the differences and sums in float64;
                       zeros when n == 0.

The gains are finite numbers (coverage gains); a NaN gain is outside the definition.

`totals` turns the per-sample arrays into one float64 vector of raw sums (counts far below 2^53: exact) that can be ADDED over
batches and ranks; `summarize_totals` forms the ratios from it: ratios of sums, never means of ratios."""
from __future__ import annotations

import math

import numpy as np

MAX_THRESHOLDS = 8
DEFAULT_THRESHOLDS = (0.13,)
# layout of the totals vector: these scalars, then (tp, fp, fn, tn) per threshold
_HEAD = ("n_samples", "n_scored", "n_targets", "n_bad_targets", "comparable", "concordant", "discordant", "hits", "sum_abs",
         "sum_sq", "sum_regret")
N_HEAD = len(_HEAD)


def check_thresholds(thresholds):
    """-> a tuple of 1..8 Python floats (ValueError otherwise; a NaN is not a threshold)."""
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    try:
        ts = tuple(thresholds)
    except TypeError:
        raise ValueError(f"thresholds: 1 to {MAX_THRESHOLDS} numbers expected, got {thresholds!r}") from None
    if not 1 <= len(ts) <= MAX_THRESHOLDS or any(isinstance(t, bool) or not isinstance(t, (int, float, np.floating, np.integer))
                                                 or math.isnan(float(t)) for t in ts):
        raise ValueError(f"thresholds: 1 to {MAX_THRESHOLDS} numbers expected, got {thresholds!r}")
    return tuple(float(t) for t in ts)


def totals_size(n_thresholds):
    return N_HEAD + 4 * int(n_thresholds)


def validation_metrics_reference(out1, out2, gt, coords, gains, bidx, thresholds):
    """One validation batch -> (obst int64 [B,T,4], rank int64 [B,6], val float64 [B,4]); see the module's docstring.
    out1 [B,8,V,V], out2 / gt [B,1,S,S] fp32 with V = S / 4; coords [K,3] int64 (heading, row, col); gains [K] fp32; bidx [K] int64,
    in any order; an index outside [0,B) belongs to no sample."""
    ts = check_thresholds(thresholds)
    out1 = np.asarray(out1, dtype=np.float32)
    out2 = np.asarray(out2, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    gains = np.asarray(gains, dtype=np.float32).reshape(-1)
    bidx = np.asarray(bidx, dtype=np.int64).reshape(-1)
    B, V = out1.shape[0], out1.shape[-1]
    S = out2.shape[-1]
    if out1.shape != (B, 8, V, V) or out2.shape != (B, 1, S, S) or gt.shape != out2.shape or S != 4 * V:
        raise ValueError("validation_metrics_reference: out1 [B,8,S/4,S/4], out2 and gt [B,1,S,S] expected")
    if not len(coords) == len(gains) == len(bidx):
        raise ValueError("validation_metrics_reference: coords [K,3], gains [K] and bidx [K] expected")
    obst = np.zeros((B, len(ts), 4), np.int64)
    rank = np.zeros((B, 6), np.int64)
    val = np.zeros((B, 4), np.float64)
    label = gt[:, 0] > np.float32(0.5)
    with np.errstate(invalid="ignore"):
        for t, tau in enumerate(ts):
            pred = out2[:, 0] >= np.float32(tau)
            obst[:, t, 0] = (pred & label).sum(axis=(1, 2))
            obst[:, t, 1] = (pred & ~label).sum(axis=(1, 2))
            obst[:, t, 2] = (~pred & label).sum(axis=(1, 2))
            obst[:, t, 3] = (~pred & ~label).sum(axis=(1, 2))
        for b in range(B):
            k = np.flatnonzero(bidx == b)                         # record order
            c = coords[k]
            good = (c[:, 0] >= 0) & (c[:, 0] < 8) & (c[:, 1] >= 0) & (c[:, 1] < V) & (c[:, 2] >= 0) & (c[:, 2] < V)
            n = int(good.sum())
            rank[b, 0], rank[b, 1] = n, len(k) - n
            if n == 0:
                continue
            c = c[good]
            p = out1[b, c[:, 0], c[:, 1], c[:, 2]]
            g = gains[k][good]
            i, j = np.triu_indices(n, 1)
            differ = g[i] != g[j]
            rank[b, 2] = differ.sum()
            rank[b, 3] = (((p[i] > p[j]) & (g[i] > g[j])) | ((p[i] < p[j]) & (g[i] < g[j]))).sum()
            rank[b, 4] = (((p[i] > p[j]) & (g[i] < g[j])) | ((p[i] < p[j]) & (g[i] > g[j]))).sum()
            finite = ~np.isnan(p)
            best = 0
            if finite.any():
                best = int(np.flatnonzero(finite & (p == p[finite].max()))[0])
            gmax = g.max()
            rank[b, 5] = int(g[best] == gmax)
            d = p.astype(np.float64) - g.astype(np.float64)
            val[b] = (np.abs(d).sum(), (d * d).sum(), float(gmax), float(g[best]))
    return obst, rank, val


def totals(obst, rank, val):
    """Per-sample arrays -> the float64 vector of raw sums (totals_size(T) numbers): add the vectors of several batches, or of
    several ranks, then summarize_totals."""
    obst, rank, val = np.asarray(obst), np.asarray(rank), np.asarray(val, dtype=np.float64)
    scored = rank[:, 0] > 0
    head = [rank.shape[0], int(scored.sum()), int(rank[:, 0].sum()), int(rank[:, 1].sum()), int(rank[:, 2].sum()),
            int(rank[:, 3].sum()), int(rank[:, 4].sum()), int(rank[:, 5].sum()), float(val[:, 0].sum()), float(val[:, 1].sum()),
            float((val[scored, 2] - val[scored, 3]).sum())]
    return np.concatenate([np.asarray(head, np.float64), obst.sum(axis=0).astype(np.float64).reshape(-1)])


def _ratio(num, den):
    """num / den as a Python float; None where it is undefined (a zero denominator, a sum that is not finite)."""
    if den == 0:
        return None
    q = float(num) / float(den)
    return q if math.isfinite(q) else None


def summarize_totals(tot, thresholds):
    """The totals vector -> a dict of plain Python numbers (json.dumps takes it); a quantity without a denominator is None."""
    ts = check_thresholds(thresholds)
    tot = np.asarray(tot, dtype=np.float64).reshape(-1)
    if tot.size != totals_size(len(ts)):
        raise ValueError(f"summarize_totals: {totals_size(len(ts))} totals expected for {len(ts)} thresholds, got {tot.size}")
    h = dict(zip(_HEAD, tot[:N_HEAD].tolist()))
    mse = _ratio(h["sum_sq"], h["n_targets"])
    ties = h["comparable"] - h["concordant"] - h["discordant"]
    out = {
        "n_samples": int(h["n_samples"]), "n_targets": int(h["n_targets"]), "n_bad_targets": int(h["n_bad_targets"]),
        "value_mae": _ratio(h["sum_abs"], h["n_targets"]),
        "value_rmse": None if mse is None else math.sqrt(mse),
        "rank_accuracy": _ratio(h["concordant"] + 0.5 * ties, h["comparable"]),
        "top1_hit_rate": _ratio(h["hits"], h["n_scored"]),
        "mean_regret": _ratio(h["sum_regret"], h["n_scored"]),
        "obstacle": [],
    }
    for t, tau in enumerate(ts):
        tp, fp, fn, _tn = tot[N_HEAD + 4 * t:N_HEAD + 4 * t + 4].tolist()
        out["obstacle"].append({"threshold": tau, "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
                                "iou": _ratio(tp, tp + fp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn)})
    return out


def summarize(obst, rank, val, thresholds):
    return summarize_totals(totals(obst, rank, val), thresholds)
