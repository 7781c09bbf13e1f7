#!/usr/bin/env python
"""Cost and effect of the depth-frame filter (hipops.depth_filter / depth_filter_batch, csrc/nbp_depth_filter.hip).
    python tools/bench_depth_filter.py [--launches 200] [--warmup 10] [--rollouts 48] [--advance 20] [--steps 20] [--windows 3]
                                       [--arms off noise noise_filter] [--parent-root DIR] [--no-kernel] [--out profiles/depth_filter.json]
Two measurements:
  kernel    both radii and both launch forms on 256 x 456 frames (a slanted scene with 10 % background, through the noise model, so
            every stage of the filter has work), every effect on: the single form on the 4 frames of one move, the batch form on a
            group of 12 x 4 frames in ring slots of 12 cameras' rings, and the noise launch on the same frames in the same process
            as the yardstick.  HIP events around `launches` back-to-back calls after `warmup` untimed ones -> microseconds per call
            and per frame (median, min and max of 5 such blocks).
  rollouts  `rollouts` lock-step rollouts (bench.py's scenes and network) advanced un-timed to step `advance`, then `windows` timed
            windows of `steps` steps each -> exploration steps per second per window, in up to four arms: "parent" (everything off,
            the package of the tree at --parent-root, which is a checkout of the parent commit with its library built, in a fresh
            child process that runs first), and in this process "off", "noise" (sigma_base 0.01, sigma_quad 0.001, dropout 0.02,
            edge_threshold 2) and "noise_filter" (the same noise, then range_base 0.03, range_quad 0.003, min_support 2,
            fill_support 6, radius 1).  The last two are built with recon_metrics and view_metrics on (both evaluate once, at the
            end, outside the windows) and also report the mean final coverage, accuracy / completeness / F-score and the held-out
            views' floater / hole shares: observations on one spec and `rollouts` scenes, not a gate.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if "--root" in sys.argv:                                # the package of another tree (the "parent" arm's child process)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import torch  # noqa: E402

NOISE = {"sigma_base": 0.01, "sigma_quad": 0.001, "dropout": 0.02, "edge_threshold": 2.0}
FILTER = {"radius": 1, "range_base": 0.03, "range_quad": 0.003, "min_support": 2, "fill_support": 6}
ARMS = {"off": {}, "noise": {"depth_noise": NOISE}, "noise_filter": {"depth_noise": NOISE, "depth_filter": FILTER}}


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
    from nextbestpath_amd.utility import hipops
    H, W = 256, 456
    g = torch.Generator().manual_seed(1)
    col, row = torch.arange(W, dtype=torch.float32)[None, :], torch.arange(H, dtype=torch.float32)[:, None]
    rings = (8.0 + 12.0 * col / W + 0.01 * row)[None, None] + 4.0 * torch.rand(12, 16, 1, 1, generator=g)
    rings = rings.expand(12, 16, H, W).contiguous()
    rings[torch.rand(12, 16, H, W, generator=g) < 0.1] = -1.0
    clean, raw, out = rings.to(dev), torch.empty(12, 16, H, W, device=dev), torch.empty(12, 16, H, W, device=dev)
    hw4 = H * W * 4

    def slots(t, r):
        return [t[r].data_ptr() + k * hw4 for k in range(4, 8)]
    noise_items = [(slots(clean, r), slots(raw, r), 7 + r, [5 + 4 * r + i for i in range(4)]) for r in range(12)]
    res = {"image": [H, W], "bytes_per_frame": 8 * H * W}
    n1 = event_us(lambda: hipops.depth_noise(clean[0, 4:8], raw[0, 4:8], 7, 5, NOISE), a.launches, a.warmup)
    n48 = event_us(lambda: hipops.depth_noise_batch(noise_items, NOISE, H, W), a.launches, a.warmup)      # (fills every raw slot used)
    res["noise"] = {"single_4_frames_us": n1, "single_us_per_frame": round(n1["median"] / 4, 3),
                    "batch_12x4_frames_us": n48, "batch_us_per_frame": round(n48["median"] / 48, 3)}
    filter_items = [(slots(raw, r), slots(out, r)) for r in range(12)]
    for radius in (1, 2):
        spec = dict(FILTER, radius=radius, fill_support=6 if radius == 1 else 18)
        f1 = event_us(lambda: hipops.depth_filter(raw[0, 4:8], out[0, 4:8], spec), a.launches, a.warmup)
        f48 = event_us(lambda: hipops.depth_filter_batch(filter_items, spec, H, W), a.launches, a.warmup)
        z, f = raw[:, 4:8], out[:, 4:8]
        res[f"filter_r{radius}"] = {"spec": spec, "single_4_frames_us": f1, "single_us_per_frame": round(f1["median"] / 4, 3),
                                    "batch_12x4_frames_us": f48, "batch_us_per_frame": round(f48["median"] / 48, 3),
                                    "batch_over_noise_batch": round(f48["median"] / n48["median"], 2),
                                    "pixels_smoothed_rejected_filled": [int(((f != z) & (f > -1) & (z > -1)).sum()),
                                                                        int(((f == -1) & (z > -1)).sum()),
                                                                        int(((f > -1) & (z == -1)).sum())]}
    return res


def bench_rollouts(a, dev, options, quality):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9), strict=True)
    net = net.to(dev).eval()
    tmp = tempfile.mkdtemp(prefix="nbp_bench_filter_")
    metrics = {"recon_metrics": True, "view_metrics": True} if quality else {}      # (off passes nothing: the arm also runs on the parent)
    ros = []
    for k in range(a.rollouts):
        name = f"maze{k}"
        make_maze_scene(os.path.join(tmp, name), seed=100 + k, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=0, **options)
        ros.append(tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=8 + k, **metrics))
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
        res = {"steps_per_s": rates, "median": float(np.median(rates)), "mean_final_coverage": round(cov, 4)}
        if quality:
            rec, views = [r.reconstruction_metrics() for r in ros], [r.view_metrics() for r in ros]

            def mean(vals):
                vals = [v for v in vals if v is not None]
                return None if not vals else round(float(np.mean(vals)), 5)
            res["quality"] = {"accuracy_mean": mean(r["accuracy_mean"] for r in rec),
                              "completeness_mean": mean(r["completeness_mean"] for r in rec),
                              "fscore": {str(t["threshold"]): mean(r["thresholds"][i]["fscore"] for r in rec)
                                         for i, t in enumerate(rec[0]["thresholds"])},
                              "floater": mean(v["floater"] for v in views), "hole": mean(v["hole"] for v in views),
                              "n_points": mean(r["n_points"] for r in rec)}
    del multi, ros
    torch.cuda.empty_cache()
    return res


def parent_arm(a):
    """The "off" arm on the package of the tree at --parent-root, in a fresh child process."""
    cmd = [sys.executable, os.path.abspath(__file__), "--root", a.parent_root, "--arms", "off", "--no-kernel", "--rollouts", str(a.rollouts),
           "--advance", str(a.advance), "--steps", str(a.steps), "--windows", str(a.windows)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])["rollouts"]["off"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--advance", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--arms", nargs="*", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: adds the arm 'parent'")
    ap.add_argument("--root", default=None, help="import the package from this tree (what the 'parent' arm's child process does)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"bench": "depth_filter", "noise": NOISE, "filter": FILTER}
    if a.rollouts > 0 and a.arms:
        res["rollouts"] = {"rollouts": a.rollouts, "window": [a.advance, a.steps, a.windows]}
    if a.parent_root and "rollouts" in res:             # first, before this process opens the GPU: one process on it at a time
        res["rollouts"]["parent"] = parent_arm(a)
    assert torch.cuda.is_available(), "bench_depth_filter measures on the GPU only"
    dev = torch.device("cuda")
    if not a.no_kernel:
        res["kernel"] = bench_kernel(a, dev)
    if a.rollouts > 0:
        for arm in a.arms:
            res["rollouts"][arm] = bench_rollouts(a, dev, ARMS[arm], quality=arm != "off")
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
