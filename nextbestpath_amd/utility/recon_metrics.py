"""Reconstruction-quality metrics of a rollout's cloud against the GT surface: the definition of record (numpy, no torch).

Not in the reference.  Coverage says which share of the GT points has a reconstructed point within one radius;
these say how far the reconstructed points lie from the surface (accuracy: cloud -> GT), how far the GT points are from anything
reconstructed (completeness: GT -> cloud), their mean (Chamfer distance), and which share of either set is within a threshold of
the other (precision, recall, F-score).  Every distance is a nearest-neighbour distance truncated at `cap`.

The device path (csrc/nbp_recon.hip through hipops.nn_dist2 / recon_stats / ReconMetrics) produces raw sums and counts only; the
ratios are formed here, on the host, from those -- by the same function for the device path and for the numpy reference."""
from __future__ import annotations

import math

import numpy as np

MAX_THRESHOLDS = 8
DEFAULT_THRESHOLDS = (1.0,)          # the coverage metric's radius
DEFAULT_CAP = 5.0                    # scene units
DEFAULT_CELL = 1.0


def check_options(thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP, cell=DEFAULT_CELL):
    """-> (thresholds as a tuple of floats, cap, cell); ValueError on anything the kernels would refuse."""
    cap, cell = float(cap), float(cell)
    if not (cap > 0 and math.isfinite(cap)) or not (cell > 0 and math.isfinite(cell)):
        raise ValueError("recon metrics: cap and cell must be positive and finite")
    try:
        ts = tuple(float(t) for t in thresholds)
    except TypeError:
        raise ValueError("recon metrics: thresholds must be a sequence of numbers") from None
    if not 1 <= len(ts) <= MAX_THRESHOLDS:
        raise ValueError(f"recon metrics: 1 to {MAX_THRESHOLDS} thresholds expected, got {len(ts)}")
    for t in ts:
        if not (t > 0 and math.isfinite(t)):
            raise ValueError("recon metrics: thresholds must be positive and finite")
        if t > cap:
            raise ValueError(f"recon metrics: threshold {t} above the cap {cap} (every distance is truncated there)")
    return ts, cap, cell


def option_spec(option):
    """The planning option `recon_metrics` -> None (off) or the keyword dict of hipops.ReconMetrics: None / False = off, True = the
    defaults, a dict with any of `thresholds`, `cap`, `cell` and `curve` (bool: the per-step curve as well; whoever passes the spec to
    hipops.ReconMetrics strips that key first, metrics_kwargs)."""
    if option is None or option is False:
        return None
    if option is True:
        option = {}
    if not isinstance(option, dict) or set(option) - {"thresholds", "cap", "cell", "curve"}:
        raise ValueError("recon_metrics: None, True or a dict with the keys thresholds / cap / cell / curve expected")
    if not isinstance(option.get("curve", False), bool):
        raise ValueError("recon_metrics: curve must be true or false")
    ts, cap, cell = check_options(option.get("thresholds", DEFAULT_THRESHOLDS), option.get("cap", DEFAULT_CAP),
                                  option.get("cell", DEFAULT_CELL))
    spec = {"thresholds": ts, "cap": cap, "cell": cell}
    if option.get("curve", False):  # the per-step curve (CurveReference / hipops.ReconCurve); the key is there only when it is on
        spec["curve"] = True
    return spec


def metrics_kwargs(spec):
    """A normalised spec without the keys that hipops.ReconMetrics / ReconCurve do not take (`curve`)."""
    return {k: v for k, v in spec.items() if k != "curve"}


def grown_box(bbox_lo, bbox_hi, cap):
    """The box of both directions: the GT bounds grown by cap, in fp32.  A point outside it is farther than cap from every GT point:
    as a target it cannot change a truncated distance, as a query its distance is cap either way."""
    lo = (np.asarray(bbox_lo, np.float32) - np.float32(cap)).astype(np.float32)
    hi = (np.asarray(bbox_hi, np.float32) + np.float32(cap)).astype(np.float32)
    return lo, hi


def sq_below(thr):
    """Largest float32 x with sqrt_fp32(x) < thr (thr > 0 finite): `d2 <= sq_below(thr)` is `sqrt(d2) < thr` decided on the squared
    distance (sqrt is monotone and correctly rounded on both sides)."""
    thr = np.float32(thr)
    x = np.float32(thr * thr)
    while np.sqrt(x) >= thr:
        x = np.nextafter(x, np.float32(0))
    while np.sqrt(np.nextafter(x, np.float32(np.inf))) < thr:
        x = np.nextafter(x, np.float32(np.inf))
    return np.float32(x)


def nn_dist2_reference(q, t, lo, hi, cap, chunk=1 << 22):
    """Brute force, fp32: d2[i] = min(cap2, min over the targets j inside the box of ((ex ex + ey ey) + ez ez)), e = t_j - q_i, every
    operation rounded to fp32, cap2 = fl(cap cap).  Inside the box: lo <= t <= hi on the three axes, in fp32 (a NaN is outside).
    A distance that is NaN (a NaN query) never lowers the minimum.  `chunk` = pair tests held in memory at once."""
    q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1, 3))
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    cap2 = np.float32(cap) * np.float32(cap)
    with np.errstate(invalid="ignore"):
        t = t[np.all((t >= lo) & (t <= hi), axis=1)]
    out = np.full(q.shape[0], cap2, np.float32)
    if t.shape[0] == 0 or q.shape[0] == 0:
        return out
    tx, ty, tz = t[:, 0][None, :], t[:, 1][None, :], t[:, 2][None, :]
    rows = max(1, int(chunk) // t.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, q.shape[0], rows):
            qq = q[i0:i0 + rows]
            ex, ey, ez = tx - qq[:, 0:1], ty - qq[:, 1:2], tz - qq[:, 2:3]
            d = (ex * ex + ey * ey) + ez * ez
            assert d.dtype == np.float32
            out[i0:i0 + rows] = np.fmin(np.fmin.reduce(d, axis=1), cap2)
    return out


def stats_reference(d2, thresholds):
    """-> (sums float64 [2] = (sum sqrt(d2), sum d2) with the square root in float64, counts int64 [T] = #{sqrt_fp32(d2) < t})."""
    d2 = np.asarray(d2, np.float32).reshape(-1)
    d = d2.astype(np.float64)
    sums = np.array([np.sqrt(d).sum(), d.sum()], np.float64)
    root = np.sqrt(d2)
    counts = np.array([int(np.count_nonzero(root < np.float32(t))) for t in thresholds], np.int64)
    return sums, counts


RAW_HEAD = 6                         # raw vector: acc sums (2), comp sums (2), n_rec, n_gt, then T acc counts and T comp counts


def pack_raw(acc_sums, acc_counts, n_rec, comp_sums, comp_counts, n_gt):
    """The raw numbers of one evaluation as ONE float64 vector [6 + 2 T] (counts below 2^53 are exact): what travels between ranks."""
    return np.concatenate([np.asarray(acc_sums, np.float64).reshape(2), np.asarray(comp_sums, np.float64).reshape(2),
                           np.array([n_rec, n_gt], np.float64), np.asarray(acc_counts, np.float64).reshape(-1),
                           np.asarray(comp_counts, np.float64).reshape(-1)])


def summarise_raw(raw, thresholds, cap):
    raw = np.asarray(raw, np.float64).reshape(-1)
    T = len(thresholds)
    if raw.shape[0] != RAW_HEAD + 2 * T:
        raise ValueError(f"recon metrics: a raw vector of {RAW_HEAD + 2 * T} numbers expected, got {raw.shape[0]}")
    return summarise(raw[0:2], raw[RAW_HEAD:RAW_HEAD + T], raw[4], raw[2:4], raw[RAW_HEAD + T:], raw[5], thresholds, cap)


def summarise(acc_sums, acc_counts, n_rec, comp_sums, comp_counts, n_gt, thresholds, cap):
    """Raw sums and counts -> the metrics.  Accuracy is cloud -> GT over the n_rec reconstructed points, completeness GT -> cloud over
    the n_gt GT points, both truncated at cap; a ratio without a denominator is None (never NaN: the dict goes into JSON)."""
    n_rec, n_gt = int(n_rec), int(n_gt)

    def mean(s, n):
        return float(s) / n if n > 0 else None

    def rmse(s, n):
        return math.sqrt(float(s) / n) if n > 0 else None

    acc, comp = mean(acc_sums[0], n_rec), mean(comp_sums[0], n_gt)
    rows = []
    for k, t in enumerate(thresholds):
        p = float(int(acc_counts[k])) / n_rec if n_rec > 0 else None
        r = float(int(comp_counts[k])) / n_gt if n_gt > 0 else None
        if p is None or r is None:
            f = None
        else:
            f = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
        rows.append({"threshold": float(t), "precision": p, "recall": r, "fscore": f})
    return {"n_points": n_rec, "n_gt": n_gt, "cap": float(cap),
            "accuracy_mean": acc, "accuracy_rmse": rmse(acc_sums[1], n_rec),
            "completeness_mean": comp, "completeness_rmse": rmse(comp_sums[1], n_gt),
            "chamfer": (acc + comp) / 2.0 if acc is not None and comp is not None else None,
            "thresholds": rows}


def reference(cloud, gt, thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP):
    """The same dict entirely in numpy: brute-force nearest neighbours in both directions inside the GT bounds grown by cap."""
    ts, cap, _ = check_options(thresholds, cap)
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    gt = np.asarray(gt, np.float32).reshape(-1, 3)
    if gt.shape[0] < 1:
        raise ValueError("recon metrics: an empty GT surface")
    lo, hi = grown_box(gt.min(0), gt.max(0), cap)
    acc_sums, acc_counts = stats_reference(nn_dist2_reference(cloud, gt, lo, hi, cap), ts)
    comp_sums, comp_counts = stats_reference(nn_dist2_reference(gt, cloud, lo, hi, cap), ts)
    return summarise(acc_sums, acc_counts, cloud.shape[0], comp_sums, comp_counts, gt.shape[0], ts, cap)


# ---- the per-step curve: the same metrics after every step, updated incrementally
class CurveReference:
    """The definition of the per-step curve (numpy; the device path is hipops.ReconCurve).  The cloud is append-only and the GT
    fixed, so both directions are incremental and equal the whole-cloud definition: a point's nearest GT distance never changes
    (accuracy: each point is queried once, in the update that appends it; sums and counts accumulate), and the minimum over a union
    is the minimum of the minima (completeness: a running per-GT-point minimum is lowered by the new points only).

    State: d2_gt fp32 [G] in the GT's order (fl(cap cap) at the start), acc_sums float64 [2], acc_counts int64 [T], n_rec."""

    def __init__(self, gt, thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP, bbox=None):
        self.thresholds, self.cap, _ = check_options(thresholds, cap)
        self.gt = np.ascontiguousarray(np.asarray(gt, np.float32).reshape(-1, 3))
        if self.gt.shape[0] < 1:
            raise ValueError("recon metrics: an empty GT surface")
        bbox = (self.gt.min(0), self.gt.max(0)) if bbox is None else bbox
        self.lo, self.hi = grown_box(bbox[0], bbox[1], self.cap)       # exactly as reference() forms it
        self.reset()

    def reset(self):
        T = len(self.thresholds)
        self.d2_gt = np.full(self.gt.shape[0], np.float32(self.cap) * np.float32(self.cap), np.float32)
        self.acc_sums, self.acc_counts, self.n_rec = np.zeros(2, np.float64), np.zeros(T, np.int64), 0
        self.rows = []

    def update(self, new_points):
        """Appends `new_points` [n,3] (n = 0: the previous row again) -> the row: pack_raw's float64 vector [6 + 2 T]."""
        new = np.asarray(new_points, np.float32).reshape(-1, 3)
        if new.shape[0]:
            sums, counts = stats_reference(nn_dist2_reference(new, self.gt, self.lo, self.hi, self.cap), self.thresholds)
            self.acc_sums = self.acc_sums + sums
            self.acc_counts = self.acc_counts + counts
            self.n_rec += new.shape[0]
            self.d2_gt = np.fmin(self.d2_gt, nn_dist2_reference(self.gt, new, self.lo, self.hi, self.cap))
        row = pack_raw(self.acc_sums, self.acc_counts, self.n_rec, *stats_reference(self.d2_gt, self.thresholds), self.gt.shape[0])
        self.rows.append(row)
        return row


def curve_auc(values, dx=1 / 40):
    """long_term_utils.compute_auc's rule (the coverage `auc`: the trapezoid rule with step dx plus y[0] dx / 2; repeated here, this
    module imports no torch) over a list; None where the list holds a None (a ratio without a denominator) or is empty."""
    if not values or any(v is None for v in values):
        return None
    y = np.asarray(values, np.float64)
    trap = getattr(np, "trapezoid", None) or np.trapz
    return float(trap(y, dx=dx) + y[0] * dx / 2.0)


def summarise_curve(rows, thresholds, cap, dx=1 / 40):
    """Raw rows [n][6 + 2 T] -> a JSON-safe dict of lists, one entry per row, every entry from summarise_raw: n_points,
    accuracy_mean, accuracy_rmse, completeness_mean, completeness_rmse, chamfer, thresholds = [{threshold, precision, recall,
    fscore}] (each a list), and auc = {"recall": [per threshold], "fscore": [...]} over the rows.  None where a ratio has no
    denominator, and for an AUC over a list that holds one; never a NaN."""
    ts = [float(t) for t in thresholds]
    rows = np.asarray(rows, np.float64).reshape(-1, RAW_HEAD + 2 * len(ts))
    per = [summarise_raw(r, ts, cap) for r in rows]
    out = {k: [p[k] for p in per] for k in ("n_points", "accuracy_mean", "accuracy_rmse", "completeness_mean", "completeness_rmse",
                                            "chamfer")}
    out["thresholds"] = [{"threshold": t, **{k: [p["thresholds"][i][k] for p in per] for k in ("precision", "recall", "fscore")}}
                         for i, t in enumerate(ts)]
    out["auc"] = {k: [curve_auc(block[k], dx) for block in out["thresholds"]] for k in ("recall", "fscore")}
    return out
