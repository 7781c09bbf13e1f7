#!/usr/bin/env python
"""Time of the training objective on one batch: the fused per-sample objective (tr.loss_weighted: csrc/nbp_objective.hip) against
the existing path (tr.gather_values + tr.loss: a gather and two MeanLossFn), forward + backward, on the same tensors.
    python tools/bench_objective.py [--reps 30] [--warmup 5] [--batch 32] [--grid 256] [--targets 20] [--out profiles/objective.json]
Every arm gets `warmup` untimed calls; then `reps` (>= 20) rounds time one call of each arm in turn, each call between two HIP
events recorded from an idle stream (so a call's own launch gaps and, in the existing path, its two host synchronisations count);
the median is the figure, min and max beside it.
The inputs are leaves (out1, out2 as the network's heads would give them): no network runs inside the timed region.  The launch
counts come from torch's profiler (kernels and memsets on the device during ONE forward + backward), torch's own small kernels
(divisions, casts, the log-variance expression) included.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks import training as tr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--targets", type=int, default=20, help="mean number of value targets per sample (K ~ batch x targets)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the figure is a median)")
    assert torch.cuda.is_available(), "bench_objective measures on the GPU only"
    dev = torch.device("cuda")
    B, S, V = a.batch, a.grid, a.grid // 4
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 2 * a.targets + 1, B)
    K = int(counts.sum())
    out1 = torch.from_numpy(rng.normal(size=(B, 8, V, V)).astype(np.float32)).to(dev).requires_grad_(True)
    out2 = torch.from_numpy(rng.uniform(0.01, 0.99, size=(B, 1, S, S)).astype(np.float32)).to(dev).requires_grad_(True)
    gt = torch.from_numpy((rng.random((B, 1, S, S)) < 0.1).astype(np.float32)).to(dev)
    coords = torch.from_numpy(np.stack([rng.integers(0, 8, K), rng.integers(0, V, K), rng.integers(0, V, K)], 1).astype(np.int64)).to(dev)
    gains = torch.from_numpy(rng.uniform(0, 5, K).astype(np.float32)).to(dev)
    bidx = torch.from_numpy(np.repeat(np.arange(B), counts).astype(np.int64)).to(dev)
    weights = torch.from_numpy(rng.uniform(0.2, 1.0, B).astype(np.float32)).to(dev)
    net = types.SimpleNamespace(log_vars=torch.nn.Parameter(torch.zeros(2, device=dev)))

    def run(loss):
        out1.grad = out2.grad = net.log_vars.grad = None
        loss.backward()

    arms = {
        "existing_gather_mse_bce": lambda: run(tr.loss(net, tr.gather_values(out1, bidx, coords), gains, out2, gt)),
        "fused_objective": lambda: run(tr.loss_weighted(net, out1, bidx, coords, gains, out2, gt)[0]),
        "fused_objective_weighted": lambda: run(tr.loss_weighted(net, out1, bidx, coords, gains, out2, gt, weights)[0]),
    }
    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(a.reps):                                       # the arms alternate: a drift of the box meets all of them
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3)
    res = {name: {"median_us": round(float(np.median(v)), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
           for name, v in us.items()}
    print("timings:", json.dumps(res), file=sys.stderr, flush=True)
    own_names = ("partial_kernel", "finish_kernel", "backward_kernel", "loss_partial", "loss_grad", "sum_doubles", "gather_values",
                 "scatter_values")
    for name, fn in arms.items():                                 # the counts, behind every timing (tracing slows the host)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        if not dev_events:
            raise RuntimeError("the profiler recorded no device activity: no launch count")
        copies = sum(1 for e in dev_events if "memcpy" in e.name.lower())
        fills = sum(1 for e in dev_events if "memset" in e.name.lower())
        res[name].update(device_activities=len(dev_events), kernels=len(dev_events) - copies - fills, fills=fills, copies=copies,
                         kernels_of_this_library=sum(1 for e in dev_events if any(s in e.name for s in own_names)))
    t_old, t_new = res["existing_gather_mse_bce"]["median_us"], res["fused_objective"]["median_us"]
    planes = B * S * S * 4
    out = {"metric": "training objective forward + backward on one batch", "B": B, "S": S, "K": K, "reps": a.reps, "warmup": a.warmup,
           "timer": "HIP events around each call from an idle stream; median", "results": res,
           "fused_over_existing": round(t_new / t_old, 3),
           "floor_bytes": 5 * planes, "fused_floor_bytes_per_time_TBps": round(5 * planes / t_new / 1e6, 3)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
