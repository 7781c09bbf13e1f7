#!/usr/bin/env python
"""Does a light 256-thread workgroup fit beside two resident convolution workgroups?  (GPU box; tools/probes/slack_probe.hip)

The B = 24 split forward runs on one stream (the path of tools/bench_forward.py --split --batch 24 --size 256); a latency-bound
filler kernel of a chosen register / LDS footprint is launched back to back on a second stream for the same span, one 256-thread
workgroup per CU and launch.  Per footprint: the forward's ms and the filler's us per launch; the forward alone three times for
the spread.
    python tools/diag/slack_probe.py [--reps 40] [--iters 300] [--rounds 2] [--out profiles/r08/slack_probe.txt]"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from nextbestpath_amd import _lib  # noqa: E402
from nextbestpath_amd import build as nbuild  # noqa: E402
from nextbestpath_amd.networks import packing  # noqa: E402
from nextbestpath_amd.utility.synthetic import make_count_maps, make_nbp_state_dict  # noqa: E402

SRC = os.path.join(ROOT, "tools", "probes", "slack_probe.hip")
SO = os.path.join(ROOT, "tools", "probes", "libslack_probe.so")
CASES = [(24, 0), (32, 0), (32, 16), (40, 0), (48, 0), (56, 0), (64, 0), (32, 24), (24, 16), (40, 16), (64, 24)]
LIVE = {24: 16, 32: 24, 40: 32, 48: 40, 56: 48, 64: 56}       # SLACK_LIVE_* of the probe


def compile_probe():
    """Builds the probe and returns {(LIVE, lds bytes): (vgprs, lds bytes)} from the compiler's resource-usage remark."""
    cmd = [nbuild._hipcc(), "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", SO]
    err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    table, key = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*slack_filler_kernelILi(\d+)ELi(\d+)E", line)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            table[key] = [None, None]
        m = re.search(r"remark:\s+VGPRs: (\d+)", line)
        if m and key:
            table[key][0] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and key:
            table[key][1] = int(m.group(1))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=300, help="dependent loads per lane and filler launch")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2, help="passes over the footprints; every second pass runs them in reverse order")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    usage = compile_probe()
    P = C.CDLL(SO)
    P.slack_filler_launch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    P.slack_filler_launch.restype = C.c_int
    L = _lib.lib()
    dev = torch.device("cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    packed = packing.pack_state_dict(make_nbp_state_dict(9), dev, precision="fp32_split")
    B, S = a.batch, a.size
    x = make_count_maps(B, S, seed=1).to(dev)
    o1 = torch.empty(B, 8, S // 4, S // 4, device=dev)
    o2 = torch.empty(B, 1, S, S, device=dev)
    nws = getattr(L, packing._FWD["fp32_split"][1])(B, S)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    fwd = getattr(L, packing._FWD["fp32_split"][0])
    # 64 MiB ring of random indices: every hop of a chain is an HBM (or at best L2) round trip
    n = 1 << 24
    g = torch.Generator().manual_seed(3)
    ring = torch.randint(0, n, (n,), generator=g, dtype=torch.int32).to(dev)
    sink = torch.empty(cus * 256, dtype=torch.int32, device=dev)
    s_fwd, s_fill = torch.cuda.Stream(), torch.cuda.Stream()

    def forward():
        _lib.check(fwd(packed.handle, x.data_ptr(), B, S, o1.data_ptr(), o2.data_ptr(), ws.data_ptr(), ws.numel(), s_fwd.cuda_stream),
                   "forward")

    def filler(regs, lds):
        rc = P.slack_filler_launch(regs, lds, ring.data_ptr(), n, a.iters, sink.data_ptr(), cus, s_fill.cuda_stream)
        assert rc == 0, rc

    def timed(case, per_forward):
        """reps forwards on s_fwd; per_forward filler launches enqueued on s_fill after each forward's launches (the host runs ahead of
        the device, so both queues stay full).  -> (ms per forward, us per filler launch or None)"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record(s_fwd)
        if case:
            ev[2].record(s_fill)
        for _ in range(a.reps):
            forward()
            for _ in range(per_forward if case else 0):
                filler(*case)
        ev[1].record(s_fwd)
        if case:
            ev[3].record(s_fill)
        torch.cuda.synchronize()
        f_ms = ev[0].elapsed_time(ev[1]) / a.reps
        return f_ms, (ev[2].elapsed_time(ev[3]) * 1e3 / (a.reps * per_forward) if case else None)

    for _ in range(3):
        forward()
    lines = [f"slack probe: split forward B={B} S={S}, {a.reps} forwards per row; filler = {cus} workgroups x 256 threads per launch, "
             f"{a.iters} dependent loads per lane", f"device: {torch.cuda.get_device_properties(0).name}"]
    alone = [timed(None, 0)[0] for _ in range(3)]
    spread = max(alone) - min(alone)
    mean_alone = sum(alone) / 3
    lines.append("forward alone, ms: " + "  ".join(f"{v:.3f}" for v in alone) + f"   mean {mean_alone:.3f}  spread {spread:.3f}")
    lines.append(f"{'filler (VGPRs alloc, LDS KB)':30s} {'compiler VGPRs':>14s} {'LDS B':>7s} {'filler alone us':>16s} {'fwd beside ms':>14s} "
                 f"{'vs alone':>9s} {'filler beside us':>17s}")
    res = {}
    order = [c for r in range(a.rounds) for c in (CASES if r % 2 == 0 else CASES[::-1])]
    for regs, lds in order:
        v, l = usage[(LIVE[regs], lds * 1024)]
        alloc = (v + 7) // 8 * 8
        # the filler alone, to size the number of launches that spans a forward
        for _ in range(3):
            filler(regs, lds)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s_fill)
        for _ in range(20):
            filler(regs, lds)
        e1.record(s_fill)
        torch.cuda.synchronize()
        us_alone = e0.elapsed_time(e1) * 1e3 / 20
        per_forward = max(1, int(mean_alone * 1e3 / us_alone))
        f_ms, us_beside = timed((regs, lds), per_forward)
        res[(regs, lds)] = max(f_ms, res.get((regs, lds), 0.0))      # the decision takes each footprint's worst pass
        lines.append(f"({alloc:3d}, {lds:2d}){'':21s} {v:14d} {l:7d} {us_alone:16.1f} {f_ms:14.3f} {f_ms / mean_alone:9.3f} {us_beside:17.1f}")
    light = max(res[(32, 0)], res[(32, 16)])
    heavy = res[(40, 0)]
    lines.append(f"decision: forward beside (32, <= 16 KB) {light:.3f} ms, beside (40, 0) {heavy:.3f} ms, alone {mean_alone:.3f} ms; "
                 f"difference {heavy - light:+.3f} ms = {(heavy - light) / spread if spread > 0 else float('inf'):.1f} x the spread of the alone runs "
                 f"({spread:.3f} ms): the idea {'stands' if heavy - light > 3 * spread and light - mean_alone < heavy - light else 'does not stand'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
