#!/usr/bin/env python
"""Time and exploration quality of the information-gain policy (testers/frontier_policy.py::InfoGainPolicy, csrc/nbp_infogain.hip;
DESIGN.md 4o), beside the frontier policy's.
    python tools/bench_infogain.py [--poses 100] [--scenes 8] [--rollouts 48] [--steps 30] [--launches 30] [--warmup 5]
                                   [--no-random-walk] [--out profiles/r12/infogain.json]
Arms:
    kernel B24_S256, B8_S512   HIP-event time of hipops.infogain_policy (five launches) on map stacks of a real rollout's density,
                               beside hipops.frontier_policy on the same stacks and a device-to-device copy of the same maps6 bytes,
                               from an idle stream, the three alternating call by call.  radius 24 and 31.
    lockstep                   rollout-steps/s of `rollouts` rollouts in one MultiRollout under infogain, frontier and the synthetic
                               explorer network, `steps` timed steps after 5 untimed ones, same scenes
    quality                    final coverage and AUC over `scenes` synthetic simple mazes (tools/bench_frontier.py's: cells 10, size
                               6.0), `poses` steps each: infogain and frontier at their defaults, the network with
                               make_explorer_state_dict(9), the random-walk driver (its own scene-coverage measure: read it as a
                               floor, not as the same quantity), and infogain over radius, distance_penalty and `unknown`
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_frontier import summarise, synthetic_stacks, timed  # noqa: E402
from nextbestpath_amd.utility import hipops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-random-walk", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "infogain.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_infogain measures on the GPU only"
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers.frontier_policy import make_policy
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    dev = torch.device("cuda")
    out = {"metric": "infogain policy: time beside the frontier policy and a copy of its input, lock-step rate, exploration quality",
           "timer": "HIP events around each call from an idle stream; infogain, frontier and copy alternate call by call",
           "launches": a.launches, "warmup": a.warmup, "poses": a.poses}

    # ---- the policy beside the frontier policy and a copy of its input
    kernel = {}
    for B, S in ((24, 256), (8, 512), (48, 256)):
        maps = synthetic_stacks(B, S, seed=B + S).to(dev)
        dst = torch.empty_like(maps)
        bufs = (torch.empty(B, 8, S // 4, S // 4, device=dev), torch.empty(B, 1, S, S, device=dev))
        bufs_f = (torch.empty_like(bufs[0]), torch.empty_like(bufs[1]))
        res = timed({"infogain": lambda: hipops.infogain_policy(maps, 24, 2, "free", 0, out=bufs),
                     "infogain_r31": lambda: hipops.infogain_policy(maps, 31, 2, "free", 0, out=bufs),
                     "frontier": lambda: hipops.frontier_policy(maps, 24, 2, "free", 0, out=bufs_f),
                     "copy": lambda: dst.copy_(maps)}, a.launches, a.warmup)
        o1 = hipops.infogain_policy(maps, 24, 2, "free", 0)[0]
        f1 = hipops.frontier_policy(maps, 24, 2, "free", 0)[0]
        kernel[f"B{B}_S{S}"] = dict(res, maps6_bytes=maps.numel() * 4, value_cells=B * (S // 4) ** 2,
                                    ratio_infogain_over_copy=round(res["infogain"]["median_us"] / res["copy"]["median_us"], 2),
                                    ratio_infogain_over_frontier=round(res["infogain"]["median_us"] / res["frontier"]["median_us"], 2),
                                    cells_with_gain=int((o1.sum(1) > 0).sum()), cells_with_frontier_value=int((f1.sum(1) > 0).sum()),
                                    mean_gain_of_those=round(float(o1.sum(1)[o1.sum(1) > 0].mean()), 1))
    out["kernel"] = kernel
    print("[bench_infogain] kernel", json.dumps(kernel), file=sys.stderr, flush=True)

    # ---- scenes
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    tmp = tempfile.mkdtemp(prefix="nbp_bench_infogain_")
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
        for label, actor in (("infogain", make_policy("infogain")), ("frontier", make_policy("frontier")), ("nbp", net)):
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
            print(f"[bench_infogain] lockstep {label}", json.dumps(lock[label]), file=sys.stderr, flush=True)
    lock["infogain_at_least_nbp"] = lock["infogain"]["rollout_steps_per_s"] >= lock["nbp"]["rollout_steps_per_s"]
    out["lockstep"] = lock

    # ---- exploration quality
    quality = {}
    with torch.no_grad():
        for label, spec in (("infogain_default", "infogain"), ("frontier_default", "frontier"), ("nbp_explorer_state_dict_9", None)):
            quality[label] = summarise(tp.run_many(params, net, ds, runs, dev, seeds, n_poses=a.poses, policy=spec))
            print(f"[bench_infogain] quality {label}", json.dumps(quality[label]), file=sys.stderr, flush=True)
        sweep = {}
        if not a.no_sweep:
            for radius, pen, unknown in ((16, 0, "free"), (31, 0, "free"), (24, 1, "free"), (24, 0, "obstacle")):
                spec = {"name": "infogain", "radius": radius, "distance_penalty": pen, "unknown": unknown}
                s = summarise(tp.run_many(params, net, ds, runs, dev, seeds, n_poses=a.poses, policy=spec))
                key = f"radius{radius}_penalty{pen}_{unknown}"
                sweep[key] = {k: s[k] for k in ("final_coverage_mean", "auc_mean")}
                print(f"[bench_infogain] {key}", json.dumps(sweep[key]), file=sys.stderr, flush=True)
        quality["sweep"] = sweep
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
