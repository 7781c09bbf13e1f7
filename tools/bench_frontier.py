#!/usr/bin/env python
"""Time and exploration quality of the frontier policy (testers/frontier_policy.py, csrc/nbp_frontier.hip).
    python tools/bench_frontier.py [--poses 100] [--scenes 8] [--rollouts 48] [--steps 30] [--launches 30] [--warmup 5]
                                   [--no-random-walk] [--out profiles/r11/frontier.json]
Arms:
    policy_B24_S256, policy_B8_S512   HIP-event time of hipops.frontier_policy (five launches) on map stacks of a real rollout's
                                      density, beside copy_*: a device-to-device copy of the same maps6 bytes, from an idle stream,
                                      the two alternating call by call.  The policy is bound by reading its input; `ratio` = policy / copy.
    lockstep                          steps/s of `rollouts` rollouts in one MultiRollout under the policy (and, beside it, under the
                                      synthetic explorer network), `steps` timed steps after 5 untimed ones
    quality                           final coverage and AUC over `scenes` synthetic simple mazes (tools/make_synthetic_dataset.py's
                                      kind: cells 10, size 6.0), `poses` steps each: the frontier policy at its defaults, the network
                                      with make_explorer_state_dict(9), the random-walk driver (its own scene-coverage measure: read
                                      it as a floor, not as the same quantity), and a sweep of the policy over radius and
                                      distance_penalty
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextbestpath_amd.utility import hipops  # noqa: E402


def timed(fns, launches, warmup):
    """{name: fn} -> {name: stats in microseconds}: the arms alternate call by call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(launches):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median_us": round(float(np.median(v)), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in us.items()}


def synthetic_stacks(B, S, seed):
    """Map stacks with the structure of a rollout's: a seen disc of sub-sampled hits around the camera, walls in the band."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    m = torch.zeros(B, 6, S, S)
    for b in range(B):
        r = S * (0.15 + 0.25 * torch.rand(1, generator=g).item())
        disc = ((yy - S // 2) ** 2 + (xx - S // 2) ** 2) < r * r
        hits = disc & (torch.rand(S, S, generator=g) < 0.35)
        ch = torch.randint(0, 5, (S, S), generator=g)
        for k in range(5):
            m[b, k][hits & (ch == k)] = 1.0
        m[b, 5][hits & (torch.rand(S, S, generator=g) < 0.1)] = 1.0
    return m


def summarise(results):
    from nextbestpath_amd.utility.long_term_utils import compute_auc
    cov = [r["coverage"] for r in results]
    return {"final_coverage_mean": round(float(np.mean([c[-1] for c in cov])), 4), "auc_mean": round(float(np.mean([compute_auc(np.asarray(c, np.float32)) for c in cov])), 4),
            "final_coverage": [round(float(c[-1]), 4) for c in cov]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-random-walk", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "frontier.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frontier measures on the GPU only"
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers.frontier_policy import FrontierPolicy
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    dev = torch.device("cuda")
    out = {"metric": "frontier policy: time beside a copy of its input, lock-step rate, exploration quality",
           "timer": "HIP events around each call from an idle stream; policy and copy alternate call by call",
           "launches": a.launches, "warmup": a.warmup, "poses": a.poses}

    # ---- the policy beside a copy of its input
    kernel = {}
    for B, S in ((24, 256), (8, 512)):
        maps = synthetic_stacks(B, S, seed=B + S).to(dev)
        dst = torch.empty_like(maps)
        bufs = (torch.empty(B, 8, S // 4, S // 4, device=dev), torch.empty(B, 1, S, S, device=dev))
        res = timed({"policy": lambda: hipops.frontier_policy(maps, 24, 2, "free", 0, out=bufs), "copy": lambda: dst.copy_(maps)},
                    a.launches, a.warmup)
        nbytes = maps.numel() * 4
        kernel[f"B{B}_S{S}"] = {"maps6_bytes": nbytes, "policy": res["policy"], "copy": res["copy"],
                                "ratio_policy_over_copy": round(res["policy"]["median_us"] / res["copy"]["median_us"], 2),
                                "policy_read_GBps": round(nbytes / (res["policy"]["median_us"] * 1e-6) / 1e9, 1),
                                "frontier_pixels": int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in
                                                           hipops.frontier_mask(maps, 2).cpu().numpy().view(np.uint64).ravel()))}
    out["kernel"] = kernel
    print("[bench_frontier] kernel", json.dumps(kernel), file=sys.stderr, flush=True)

    # ---- scenes
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    tmp = tempfile.mkdtemp(prefix="nbp_bench_frontier_")
    names = [f"maze_{i:02d}" for i in range(a.scenes)]
    for i, name in enumerate(names):
        make_maze_scene(os.path.join(tmp, name), seed=i, cells=10, size=6.0, height=1.2, tess=0.25, n_starts=1, hull="slab")
    ds = sc.SceneDataset(tmp, names)
    runs = tp.list_runs(ds, params)
    seeds = [8 + 1000 * r[0] + r[1] for r in runs]
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9), strict=True)
    net = net.to(dev).eval()

    # ---- lock-step rate
    lock = {}
    with torch.no_grad():
        for label, actor in (("frontier", FrontierPolicy("frontier")), ("nbp", net)):
            ros = [tp.build_rollout(params, actor, ds, runs[k % len(runs)], dev, seed=100 + k) for k in range(a.rollouts)]
            multi = tp.MultiRollout(ros, actor, dev)
            for _ in range(5):
                multi.step()
            multi.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                multi.step()
            multi.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            lock[label] = {"rollouts": a.rollouts, "steps": a.steps, "seconds": round(dt, 4),
                           "rollout_steps_per_s": round(a.rollouts * a.steps / dt, 1)}
            del ros, multi
            torch.cuda.empty_cache()
    out["lockstep"] = lock
    print("[bench_frontier] lockstep", json.dumps(lock), file=sys.stderr, flush=True)

    # ---- exploration quality
    quality = {}
    with torch.no_grad():
        quality["frontier_default"] = summarise(tp.run_many(params, net, ds, runs, dev, seeds, n_poses=a.poses, policy="frontier"))
        quality["nbp_explorer_state_dict_9"] = summarise(tp.run_many(params, net, ds, runs, dev, seeds, n_poses=a.poses))
        sweep = {}
        for radius in (8, 16, 24, 31):
            for pen in (0, 1, 3):
                spec = {"name": "frontier", "radius": radius, "distance_penalty": pen}
                s = summarise(tp.run_many(params, net, ds, runs, dev, seeds, n_poses=a.poses, policy=spec))
                sweep[f"radius{radius}_penalty{pen}"] = {k: s[k] for k in ("final_coverage_mean", "auc_mean")}
                print(f"[bench_frontier] radius {radius} penalty {pen}", json.dumps(sweep[f"radius{radius}_penalty{pen}"]), file=sys.stderr, flush=True)
        quality["sweep"] = sweep
    print("[bench_frontier] quality", json.dumps({k: v for k, v in quality.items() if k != "sweep"}), file=sys.stderr, flush=True)
    if not a.no_random_walk:
        from nextbestpath_amd.testers.random_walk_planning import test_random_walk_planning
        res = test_random_walk_planning("macarons_default_training_config.json", None, "random_walk.json", 0, names, dataset_path=tmp,
                                        results_dir=tmp, n_poses=a.poses, seed=8)
        quality["random_walk"] = summarise([rec for scene in res.values() for rec in scene.values()])
    out["quality"] = quality
    shutil.rmtree(tmp, ignore_errors=True)

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
