#!/usr/bin/env python
"""The D4 symmetry ensemble of the eval forward (NBP.symmetry_ensemble), measured:
    python tools/bench_ensemble.py [--size 256] [--batches 1,48] [--forward-batches 1,24] [--launches 50]
  * kernel time of nbp_ensemble_expand_f32 and nbp_ensemble_reduce_f32 per ensemble and batch (HIP events around each launch after
    warm-up, same process, same buffers), the bytes each must move (every input byte read once, every output byte written once) and
    that rate as a fraction of the achievable HBM bandwidth, which is measured here too: a device-to-device copy of 1 GiB.  At
    B = 1 the kernels' few MB stay in the caches, so their "fraction" may exceed 1: it is bytes over time, not an HBM counter;
  * eval forward maps/s (input maps, not moved copies) with symmetry_ensemble None, "c2", "flips" and "d4": the eager call, and at
    B = 1 also the captured graph (NBP.forward_static), wall clock around a synchronised window;
  * packing.equivariance_error of the seeded test weights (utility/synthetic.py::make_nbp_state_dict(9)) on count maps.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks import packing  # noqa: E402
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.utility import augment, hipops  # noqa: E402
from nextbestpath_amd.utility.synthetic import make_count_maps, make_nbp_state_dict  # noqa: E402

ENSEMBLES = ("c2", "flips", "d4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", type=str, default="1,48")
    ap.add_argument("--forward-batches", type=str, default="1,24")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forwards", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    S, V = a.size, a.size // 4

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        us = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}

    big, big_o = torch.rand(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    copy = timed(lambda: big_o.copy_(big))
    copy["bytes_moved"] = 2 * 4 * (1 << 28)
    copy["GBps"] = round(copy["bytes_moved"] / copy["median_us"] / 1e3, 1)
    del big, big_o
    kernels = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.rand(B, 5, S, S, device=dev)
        for name in ENSEMBLES:
            ops = hipops.symmetry_ops(name, dev)
            n = len(augment.ENSEMBLES[name])
            xe = torch.empty(n, B, 5, S, S, device=dev)
            raw1, raw2 = torch.rand(n, B, 8, V, V, device=dev), torch.rand(n, B, 1, S, S, device=dev)
            out = (torch.empty(B, 8, V, V, device=dev), torch.empty(B, 1, S, S, device=dev))
            for kernel, fn, nbytes in (("expand", lambda: hipops.symmetry_expand(x, ops, out=xe), 4 * (1 + n) * B * 5 * S * S),
                                       ("reduce", lambda: hipops.symmetry_reduce(raw1, raw2, ops, out=out),
                                        4 * (1 + n) * B * (8 * V * V + S * S))):
                r = timed(fn)
                r.update(kernel=kernel, ensemble=name, batch=B, bytes_moved=nbytes, GBps=round(nbytes / r["median_us"] / 1e3, 1))
                r["fraction_of_copy_bandwidth"] = round(r["GBps"] / copy["GBps"], 3)
                kernels.append(r)
            del xe, raw1, raw2, out

    net = NBP()
    net.load_state_dict(make_nbp_state_dict(9), strict=True)
    net = net.to(dev).eval()
    forward = []
    with torch.no_grad():
        for B in [int(b) for b in a.forward_batches.split(",")]:
            x = make_count_maps(B, S, seed=B).to(dev)
            for name in (None,) + ENSEMBLES:
                net.symmetry_ensemble = name
                modes = [("eager", lambda: net(x))] + ([("graph", lambda: net.forward_static(x))] if B == 1 else [])
                for mode, fn in modes:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.forwards):
                        fn()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    forward.append({"ensemble": name, "batch": B, "mode": mode, "ms_per_forward": round(dt / a.forwards * 1e3, 3),
                                    "maps_per_s": round(B * a.forwards / dt, 2)})
        net.symmetry_ensemble = None
        for row in forward:
            base = next(r for r in forward if r["ensemble"] is None and (r["batch"], r["mode"]) == (row["batch"], row["mode"]))
            row["x_plain"] = round(row["ms_per_forward"] / base["ms_per_forward"], 3)
        e1, e2 = packing.equivariance_error(net, make_count_maps(1, S, seed=1).to(dev), "d4")
    print(json.dumps({"metric": "NBP symmetry ensemble", "size": S, "precision": net.conv_precision,
                      "timer": "HIP events around each launch (kernels); wall clock around a synchronised window (forwards)",
                      "copy_d2d_1GiB": copy, "kernels": kernels, "forward": forward,
                      "equivariance_error_seeded_test_weights": {"out1": e1, "out2": e2, "ops": "d4", "batch": 1}}))


if __name__ == "__main__":
    main()
