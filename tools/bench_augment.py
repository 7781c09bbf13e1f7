#!/usr/bin/env python
"""Kernel time of the D4 batch augmentation (nbp_augment_batch_f32) per op class, beside a device-to-device copy of the same bytes.
    python tools/bench_augment.py [--batch 32] [--size 256] [--launches 50]
HIP events around each launch after warm-up, same process, same buffers; the copy (6 B S^2 floats read + written) is the yardstick.
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd import _lib  # noqa: E402

CLASSES = {"identity": [0], "reflections": [2, 4, 6], "transposing": [1, 3, 5, 7], "mixed": list(range(8))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, S = a.batch, a.size
    x, gt = torch.rand(B, 5, S, S, device=dev), torch.rand(B, 1, S, S, device=dev)
    xo, go = torch.empty_like(x), torch.empty_like(gt)
    both, both_o = torch.rand(B * 6 * S * S, device=dev), torch.empty(B * 6 * S * S, device=dev)
    L = _lib.lib()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e3)
        ms.sort()
        return {"median_us": round(ms[len(ms) // 2], 2), "min_us": round(ms[0], 2), "max_us": round(ms[-1], 2)}

    nbytes = 2 * 6 * B * S * S * 4
    res = {"copy_d2d": timed(lambda: both_o.copy_(both))}
    for name, codes in CLASSES.items():
        ops = torch.tensor([codes[i % len(codes)] for i in range(B)], dtype=torch.int32, device=dev)

        def launch():
            _lib.check(L.nbp_augment_batch_f32(_lib.ptr(x), _lib.ptr(gt), _lib.ptr(ops), B, S, _lib.ptr(xo), _lib.ptr(go),
                                               _lib.current_stream()), "nbp_augment_batch_f32")
        res[name] = timed(launch)
    for v in res.values():
        v["GBps"] = round(nbytes / v["median_us"] / 1e3, 1)
        v["x_copy"] = round(v["median_us"] / res["copy_d2d"]["median_us"], 3)
    print(json.dumps({"metric": "nbp_augment_batch_f32 kernel time", "batch": B, "size": S, "bytes_moved": nbytes,
                      "launches": a.launches, "timer": "HIP events around each launch", "results": res}))


if __name__ == "__main__":
    main()
