#!/usr/bin/env python
"""Time of the validation-metrics launches (hipops.validation_metrics, csrc/nbp_metrics.hip) on one validation batch.
    python tools/bench_metrics.py [--launches 50] [--warmup 5] [--batch 32] [--grid 256] [--targets 20] [--out profiles/metrics.json]
Arms, each timed with HIP events around every call from an idle stream (so a call's own launch gaps count), `warmup` untimed calls
first, all in this process:
    a  hipops.validation_metrics: one memset + two launches; reads out2 and gt once (8 B per pixel) and the sparse targets
    b  a device-to-device copy of the same bytes (out2 + gt; a copy reads and writes them)
    c  one eval forward of the batch (what a validation batch costs without the metrics, its loss launches aside)
Prints one JSON line (and writes it to --out): per arm the median (min - max) in microseconds, a / b and a / (a + c)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.utility import hipops  # noqa: E402
from nextbestpath_amd.utility.synthetic import make_count_maps, make_nbp_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--targets", type=int, default=20, help="mean number of targets per sample")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.13])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics measures on the GPU only"
    dev = torch.device("cuda")
    B, S, V = a.batch, a.grid, a.grid // 4
    rng = np.random.default_rng(3)
    net = NBP()
    net.load_state_dict(make_nbp_state_dict(9), strict=True)
    net = net.to(dev).eval()
    xs = make_count_maps(B, S, seed=2).to(dev)
    with torch.no_grad():
        out1, out2 = (t.clone() for t in net(xs))
    gt = torch.from_numpy((rng.random((B, 1, S, S)) < 0.1).astype(np.float32)).to(dev)
    counts = rng.integers(1, 2 * a.targets, B)
    K = int(counts.sum())
    coords = torch.from_numpy(np.stack([rng.integers(0, 8, K), rng.integers(0, V, K), rng.integers(0, V, K)], 1).astype(np.int64)).to(dev)
    d = rng.integers(-2, 6, K)
    gains = torch.from_numpy(np.where(d > 0, d * 100, 0).astype(np.float32)).to(dev)
    bidx = torch.from_numpy(np.repeat(np.arange(B), counts).astype(np.int64)).to(dev)
    src = torch.cat([out2.reshape(-1), gt.reshape(-1)])
    dst = torch.empty_like(src)

    def forward():
        with torch.no_grad():
            net(xs)

    arms = {"a_validation_metrics": lambda: hipops.validation_metrics(out1, out2, gt, coords, gains, bidx, a.thresholds),
            "b_copy_of_out2_and_gt": lambda: dst.copy_(src),
            "c_eval_forward": forward}
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
    ta, tb, tc = (res[k]["median_us"] for k in arms)
    nbytes = src.numel() * 4
    out = {"metric": "validation-metrics time on one validation batch", "B": B, "S": S, "K": K, "thresholds": a.thresholds,
           "launches": a.launches, "warmup": a.warmup, "timer": "HIP events around each call from an idle stream", "results": res,
           "bytes_read": nbytes, "a_TBps": round(nbytes / ta / 1e6, 3), "a_over_copy": round(ta / tb, 3),
           "a_share_of_forward_plus_metrics": round(ta / (ta + tc), 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
