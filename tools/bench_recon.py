#!/usr/bin/env python
"""Time of the reconstruction-quality metrics (hipops.ReconMetrics, csrc/nbp_recon.hip) on a rollout-sized cloud.
    python tools/bench_recon.py [--launches 20] [--warmup 3] [--cloud 3000000] [--gt 50000] [--out profiles/recon.json]
Inputs: G GT points on a synthetic surface (a height field over a 100 x 100 square), N cloud points within ~0.3 of it plus 5 %
uniform outliers in the surface's box grown by 10; the cloud sits in a buffer of rollout capacity with its length in a device counter.
Arms, each timed with HIP events around every call from an idle stream, `warmup` untimed calls first, all in this process:
    a  cloud -> GT   the planned nearest-neighbour query (the GT sorted once, outside the timing)
    b  GT -> cloud   the cloud sorted into the grid (memset, bin, scan, scatter) and the query over the GT
    c  the two summaries (hipops.recon_stats over N and over G distances: two launches each)
    d  ReconMetrics.evaluate: a + b + c as a rollout's end runs them
    e  GT plan build (once per rollout)
Prints one JSON line (and writes it to --out): per arm the median (min - max) in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.utility import hipops  # noqa: E402


def surface(n, rng):
    x, z = rng.uniform(0, 100, n), rng.uniform(0, 100, n)
    y = 4.0 * np.sin(x * 0.21) * np.cos(z * 0.17) + 5.0
    return np.stack([x, y, z], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cloud", type=int, default=3_000_000)
    ap.add_argument("--gt", type=int, default=50_000)
    ap.add_argument("--capacity", type=int, default=3_400_000)
    ap.add_argument("--cap", type=float, default=5.0)
    ap.add_argument("--cell", type=float, default=1.0)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[1.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_recon measures on the GPU only"
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    N, G = a.cloud, a.gt
    gt_h = surface(G, rng)
    n_out = N // 20
    near = surface(N - n_out, rng) + rng.normal(0, 0.15, (N - n_out, 3)).astype(np.float32)
    lo, hi = gt_h.min(0), gt_h.max(0)
    out = rng.uniform(lo - 10, hi + 10, (n_out, 3)).astype(np.float32)
    cloud_h = np.concatenate([near, out])
    rng.shuffle(cloud_h)
    gt = torch.from_numpy(gt_h).to(dev)
    cloud = torch.zeros(max(a.capacity, N), 3, dtype=torch.float32, device=dev)
    cloud[:N] = torch.from_numpy(cloud_h).to(dev)
    n_dev = torch.tensor([N], dtype=torch.int64, device=dev)
    bbox = (lo.tolist(), hi.tolist())
    rm = hipops.ReconMetrics(gt, bbox, a.thresholds, a.cap, a.cell)
    d2c = torch.empty(cloud.shape[0], dtype=torch.float32, device=dev)
    d2g = torch.empty(G, dtype=torch.float32, device=dev)

    def stats():
        hipops.recon_stats(d2c, a.thresholds, n_dev)
        hipops.recon_stats(d2g, a.thresholds)

    arms = {"a_cloud_to_gt_planned": lambda: rm.plan.dist2(cloud, a.cap, n_query_dev=n_dev, out=d2c),
            "b_gt_to_cloud_sort_and_query": lambda: hipops.nn_dist2(gt, cloud, rm.box, a.cap, a.cell, n_target_dev=n_dev, out=d2g),
            "c_two_summaries": stats,
            "d_evaluate": lambda: rm.evaluate(cloud, n_dev),
            "e_gt_plan_build": lambda: hipops.NNPlan(gt, rm.box, a.cell)}
    res = {}
    for name, fn in arms.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        res[name] = {"median_us": round(float(np.median(us)), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}
    summary = rm.summary()
    line = json.dumps({"metric": "reconstruction-metrics time at a rollout's end", "N": N, "G": G, "capacity": cloud.shape[0],
                       "cap": a.cap, "cell": a.cell, "thresholds": a.thresholds, "launches": a.launches, "warmup": a.warmup,
                       "timer": "HIP events around each call from an idle stream", "results": res, "summary": summary})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
