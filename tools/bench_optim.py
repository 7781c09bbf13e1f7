#!/usr/bin/env python
"""Time of one optimizer step over the real NBP() parameter list (seeded gradients), HipAdamW beside torch's fused AdamW.
    python tools/bench_optim.py [--launches 50] [--warmup 5] [--rounds 3] [--clip 1.0] [--out profiles/r09/optim.json]
Arms, alternated `rounds` times in one process (each arm owns its parameters and state; HIP events around each step() from an idle
stream, so a step's own launch gaps count):
    a  torch.optim.AdamW(fused=True).step()
    b  HipAdamW.step() without the norm pass
    c  HipAdamW.step() with it (max_grad_norm, skip_nonfinite)
    d  torch.nn.utils.clip_grad_norm_ + a: the torch way of getting c
    e  a device-to-device copy of 200 MB (100 MB read + 100 MB written per 100 MB copied: the box's stream rate)
Prints one JSON line (and writes it to --out): per arm the median (min - max) over all rounds and each round's median; for b the
bytes of the update (28 B per parameter: p, g, m, v read, p, m, v written) over its time, against 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.optim import HipAdamW  # noqa: E402

KW = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim measures on the GPU only"
    dev = torch.device("cuda")
    torch.manual_seed(9)
    ref = [p.detach() for p in NBP().parameters()]
    gen = torch.Generator().manual_seed(5)
    grads = [(torch.randn(p.shape, generator=gen) * 1e-2).to(dev) for p in ref]
    n_params = sum(p.numel() for p in ref)

    def params(own_grads=False):
        ps = [torch.nn.Parameter(p.clone().to(dev)) for p in ref]
        for p, g in zip(ps, grads):
            p.grad = g.clone() if own_grads else g          # (clip_grad_norm_ scales its gradients in place: arm d owns a copy)
        return ps

    pa, pb, pc, pd = params(), params(), params(), params(own_grads=True)
    oa = torch.optim.AdamW(pa, fused=True, **KW)
    ob = HipAdamW(pb, **KW)
    oc = HipAdamW(pc, max_grad_norm=a.clip, skip_nonfinite=True, **KW)
    od = torch.optim.AdamW(pd, fused=True, **KW)
    src, dst = torch.rand(50_000_000, device=dev), torch.empty(50_000_000, device=dev)

    def clip_then_step():
        torch.nn.utils.clip_grad_norm_(pd, a.clip)
        od.step()

    arms = {"a_torch_fused": oa.step, "b_hip": ob.step, "c_hip_norm": oc.step, "d_torch_clip_fused": clip_then_step,
            "e_copy_200MB": lambda: dst.copy_(src)}
    samples = {k: [] for k in arms}
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
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
            samples[name] += us
            rounds[name].append(round(float(np.median(us)), 1))
    res = {k: {"median_us": round(float(np.median(v)), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
               "round_medians_us": rounds[k]} for k, v in samples.items()}
    b, c = res["b_hip"]["median_us"], res["c_hip_norm"]["median_us"]
    out = {"metric": "optimizer step time over the NBP parameter list", "parameters": n_params, "tensors": len(ref),
           "launches": a.launches, "warmup": a.warmup, "rounds": a.rounds, "clip": a.clip,
           "timer": "HIP events around each step() from an idle stream", "results": res,
           "b_over_a": round(b / res["a_torch_fused"]["median_us"], 3), "c_over_d": round(c / res["d_torch_clip_fused"]["median_us"], 3),
           "b_bytes": 28 * n_params, "b_TBps": round(28 * n_params / b / 1e6, 3), "b_frac_of_8TBps": round(28 * n_params / b / 1e6 / 8.0, 3),
           "e_TBps_read_plus_write": round(2 * 4 * src.numel() / res["e_copy_200MB"]["median_us"] / 1e6, 3),
           "skipped_steps": int(oc.skipped_steps), "last_grad_norm": float(oc.last_grad_norm)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
