#!/usr/bin/env python
"""Cost of the depth-sensor noise model (hipops.depth_noise / depth_noise_batch, csrc/nbp_depth_noise.hip).
    python tools/bench_depth_noise.py [--launches 200] [--warmup 10] [--rollouts 48] [--advance 20] [--steps 20] [--windows 3]
                                      [--arms off on] [--no-kernel] [--out profiles/depth_noise.json]
Two measurements, all in this process:
  kernel    the two launch forms on 256 x 456 frames of depths 1 .. 60 with 10 % background, every effect on: the single form on the 4
            frames of one move, the batch form on a group of 12 x 4 frames in ring slots of 12 cameras' rings.  HIP events around
            `launches` back-to-back calls after `warmup` untimed ones -> microseconds per call and per frame (median of 5 such blocks).
  rollouts  `rollouts` lock-step rollouts (bench.py's scenes and network) advanced un-timed to step `advance`, then `windows` timed
            windows of `steps` steps each, with the option off and on (sigma_base 0.01, sigma_quad 0.001, dropout 0.02,
            edge_threshold 2): exploration steps per second per window.  `--arms off` alone also runs on a tree from before the option.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextbestpath_amd.utility import hipops  # noqa: E402

SPEC = {"sigma_base": 0.01, "sigma_quad": 0.001, "dropout": 0.02, "edge_threshold": 2.0}


def event_us(fn, launches, warmup, blocks=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return {"median": round(float(np.median(out)), 3), "min": round(min(out), 3), "max": round(max(out), 3)}


def bench_kernel(a, dev):
    H, W = 256, 456
    g = torch.Generator().manual_seed(1)
    rings = torch.rand(12, 16, H, W, generator=g) * 59.0 + 1.0
    rings[torch.rand(12, 16, H, W, generator=g) < 0.1] = -1.0
    clean, out = rings.to(dev), torch.empty(12, 16, H, W, device=dev)
    single = event_us(lambda: hipops.depth_noise(clean[0, 4:8], out[0, 4:8], 7, 5, SPEC), a.launches, a.warmup)
    hw4 = H * W * 4
    items = [([clean[r].data_ptr() + k * hw4 for k in range(4, 8)], [out[r].data_ptr() + k * hw4 for k in range(4, 8)], 7 + r,
              [5 + 4 * r + i for i in range(4)]) for r in range(12)]
    batch = event_us(lambda: hipops.depth_noise_batch(items, SPEC, H, W), a.launches, a.warmup)
    return {"image": [H, W], "bytes_per_frame": 8 * H * W,
            "single_4_frames_us": single, "single_us_per_frame": round(single["median"] / 4, 3),
            "batch_12x4_frames_us": batch, "batch_us_per_frame": round(batch["median"] / 48, 3),
            "batch_gb_per_s": round(48 * 8 * H * W / batch["median"] / 1e3, 1)}


def bench_rollouts(a, dev, spec):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9), strict=True)
    net = net.to(dev).eval()
    tmp = tempfile.mkdtemp(prefix="nbp_bench_noise_")
    kw = {} if spec is None else {"depth_noise": spec}          # (off passes nothing: the arm also runs on a tree without the option)
    ros = []
    for k in range(a.rollouts):
        name = f"maze{k}"
        make_maze_scene(os.path.join(tmp, name), seed=100 + k, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=0, **kw)
        ros.append(tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=8 + k))
    multi = tp.MultiRollout(ros, net, dev)

    def run(n):
        for _ in range(n):
            multi.step()
        multi.flush()
    with torch.no_grad():
        run(a.advance)
        rates = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            torch.cuda.synchronize()
            rates.append(round(a.steps * a.rollouts / (time.perf_counter() - t0), 1))
    cov = float(np.mean([r.coverage_evolution(a.advance + a.windows * a.steps)[-1] for r in ros]))
    del multi, ros
    torch.cuda.empty_cache()
    return {"steps_per_s": rates, "median": float(np.median(rates)), "mean_final_coverage": round(cov, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--advance", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--arms", nargs="*", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_noise measures on the GPU only"
    dev = torch.device("cuda")
    res = {"bench": "depth_noise", "spec": SPEC}
    if not a.no_kernel:
        res["kernel"] = bench_kernel(a, dev)
    if a.rollouts > 0 and a.arms:
        res["rollouts"] = {"rollouts": a.rollouts, "window": [a.advance, a.steps, a.windows]}
        for arm in a.arms:
            res["rollouts"][arm] = bench_rollouts(a, dev, SPEC if arm == "on" else None)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
