#!/usr/bin/env python
"""Time of one weight-average update over the real NBP() tensor list (parameters and BatchNorm running statistics).
    python tools/bench_ema.py [--launches 50] [--warmup 5] [--decay 0.999] [--out profiles/r10/ema.json]
Arms, each timed with HIP events around every call from an idle stream (so a call's own launch gaps count), `warmup` untimed calls
first:
    a  WeightEMA.update()                    12 B per element: p and e read, e written
    b  WeightEMA.update(HipAdamW) behind a step the optimizer dropped: the gated-off launch (no traffic)
    c  a device-to-device copy of the same 12 B per element (a copy moves 8 B per element copied: 1.5 x the element count)
    d  torch's emulation, torch._foreach_lerp_ over the same lists (no gate, no device-side schedule)
Prints one JSON line (and writes it to --out): per arm the median (min - max) in microseconds; for a its bytes over its time."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.optim import HipAdamW, WeightEMA  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema measures on the GPU only"
    dev = torch.device("cuda")
    torch.manual_seed(9)
    net = NBP().to(dev)
    ema = WeightEMA(net, a.decay)
    live = list(net.parameters()) + [b for b in net.buffers() if b.dtype.is_floating_point]
    n_elems = sum(t.numel() for t in live)

    # arm b: an optimizer whose last step was dropped on the device (one planted inf; the parameters keep their bits)
    opt = HipAdamW(list(net.parameters()), skip_nonfinite=True)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    next(net.parameters()).grad.view(-1)[0] = float("inf")
    opt.step()
    assert int(opt.skipped_steps) == 1

    n_copy = (3 * n_elems + 1) // 2
    src, dst = torch.rand(n_copy, device=dev), torch.empty(n_copy, device=dev)
    twin = [t.detach().clone() for t in live]
    detached = [t.detach() for t in live]

    arms = {"a_hip_update": lambda: ema.update(), "b_hip_update_gated_off": lambda: ema.update(opt),
            "c_copy_12B_per_element": lambda: dst.copy_(src),
            "d_torch_foreach_lerp": lambda: torch._foreach_lerp_(twin, detached, 1.0 - a.decay)}
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
    assert int(ema.num_updates) == a.warmup + a.launches, "arm b's updates were not dropped on the device"
    t = res["a_hip_update"]["median_us"]
    out = {"metric": "weight-average update time over the NBP tensor list", "elements": n_elems, "tensors": len(live),
           "launches": a.launches, "warmup": a.warmup, "decay": a.decay, "timer": "HIP events around each call from an idle stream",
           "results": res, "a_bytes": 12 * n_elems, "a_TBps": round(12 * n_elems / t / 1e6, 3),
           "a_frac_of_8TBps": round(12 * n_elems / t / 1e6 / 8.0, 3),
           "c_TBps_read_plus_write": round(8 * n_copy / res["c_copy_12B_per_element"]["median_us"] / 1e6, 3),
           "a_over_c": round(t / res["c_copy_12B_per_element"]["median_us"], 3),
           "num_updates": int(ema.num_updates)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
