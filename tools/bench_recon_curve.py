#!/usr/bin/env python
"""Time of one update of the per-step reconstruction curve (hipops.ReconCurve, csrc/nbp_recon.hip) next to the full evaluation that
was the only way to a curve point before it (hipops.ReconMetrics.evaluate), in one session.
    python tools/bench_recon_curve.py [--launches 10] [--warmup 2] [--new 29180] [--gt 50000] [--out profiles/recon_curve.json]
Inputs: tools/bench_recon.py's synthetic set -- G GT points on a height field over a 100 x 100 square, cloud points within ~0.3 of it
plus 5 % uniform outliers in the surface's box grown by 10, in a buffer of rollout capacity with its length in a device counter.
Arms, each timed with HIP events around every call from an idle stream, `warmup` untimed calls first:
    update_seen_<S>   ONE update that takes in `new` points (5 frames x 5,836) behind a cloud of S = 0, 1 M, 3 M points; the curve's
                      state (d2_gt, totals, watermark) is put back to "S points seen" before every call, outside the timing
    batch16_seen_3M   ONE recon_curve_update_batch call over 16 curves in that state, `new` points each
    evaluate_3M       ReconMetrics.evaluate of the cloud of 3 M + `new` points: both directions over the whole cloud and their summaries
Prints one JSON line (and writes it to --out): per arm the median (min - max) in microseconds; `check`: the curve's row after the
update at 3 M equals the full evaluation's counts and completeness sums."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.utility import hipops  # noqa: E402


def surface(n, rng):
    """tools/bench_recon.py's height field."""
    x, z = rng.uniform(0, 100, n), rng.uniform(0, 100, n)
    y = 4.0 * np.sin(x * 0.21) * np.cos(z * 0.17) + 5.0
    return np.stack([x, y, z], 1).astype(np.float32)


def timed(fn, before, launches, warmup):
    us = []
    for k in range(warmup + launches):
        before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if k >= warmup:
            us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--new", type=int, default=29_180)
    ap.add_argument("--seen", type=int, nargs="+", default=[0, 1_000_000, 3_000_000])
    ap.add_argument("--gt", type=int, default=50_000)
    ap.add_argument("--capacity", type=int, default=3_400_000)
    ap.add_argument("--cap", type=float, default=5.0)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[1.0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_recon_curve measures on the GPU only"
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    G, N = a.gt, max(a.seen) + a.new
    assert N <= a.capacity
    gt_h = surface(G, rng)
    n_out = N // 20
    near = surface(N - n_out, rng) + rng.normal(0, 0.15, (N - n_out, 3)).astype(np.float32)
    lo, hi = gt_h.min(0), gt_h.max(0)
    cloud_h = np.concatenate([near, rng.uniform(lo - 10, hi + 10, (n_out, 3)).astype(np.float32)])
    rng.shuffle(cloud_h)
    gt = torch.from_numpy(gt_h).to(dev)
    cloud = torch.zeros(a.capacity, 3, dtype=torch.float32, device=dev)
    cloud[:N] = torch.from_numpy(cloud_h).to(dev)
    n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    bbox = (lo.tolist(), hi.tolist())
    rm = hipops.ReconMetrics(gt, bbox, a.thresholds, a.cap, a.cell)
    curves = [hipops.ReconCurve(gt, bbox, a.thresholds, a.cap, a.cell, n_rows=2, plan=rm.plan) for _ in range(a.batch)]
    cv = curves[0]
    res, state = {}, None
    for S in sorted(a.seen):
        # the state "S points seen": one update over the first S points (the watermark only moves forward: the sizes ascend)
        n_dev.fill_(S)
        cv.update(cloud, n_dev, 0, S)
        state = (cv.d2_gt.clone(), cv.totals.clone(), cv.seen.clone())

        def restore(targets=(cv,), state=state):
            for c in targets:
                c.d2_gt.copy_(state[0]); c.totals.copy_(state[1]); c.seen.copy_(state[2])

        n_dev.fill_(S + a.new)
        res[f"update_seen_{S}"] = timed(lambda: cv.update(cloud, n_dev, 1, a.new), restore, a.launches, a.warmup)
    S = max(a.seen)
    row = cv.rows[1].cpu().numpy()
    res[f"batch{a.batch}_seen_{S}"] = timed(
        lambda: hipops.recon_curve_update_batch([c.item(cloud, n_dev, 1, a.new) for c in curves]),
        lambda: restore(curves), a.launches, a.warmup)
    res[f"evaluate_{S}"] = timed(lambda: rm.evaluate(cloud, n_dev), lambda: None, a.launches, a.warmup)
    full = rm.raw()
    check = bool(np.array_equal(row[2:], full[2:]) and np.allclose(row[:2], full[:2], rtol=1e-12, atol=0)
                 and all(np.array_equal(c.rows[1].cpu().numpy().view(np.uint64), row.view(np.uint64)) for c in curves))
    line = json.dumps({"metric": "per-step reconstruction curve: one incremental update against the full evaluation", "G": G,
                       "new": a.new, "capacity": a.capacity, "cap": a.cap, "cell": a.cell, "thresholds": a.thresholds,
                       "launches": a.launches, "warmup": a.warmup, "timer": "HIP events around each call from an idle stream",
                       "results": res, "check": check, "summary": rm.summary()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    assert check, "the curve's row differs from the full evaluation"


if __name__ == "__main__":
    main()
