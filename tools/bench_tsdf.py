#!/usr/bin/env python
"""Cost and effect of TSDF fusion (hipops.tsdf_integrate / tsdf_integrate_batch / tsdf_extract, csrc/nbp_tsdf.hip).
    python tools/bench_tsdf.py [--launches 100] [--warmup 5] [--rollouts 48] [--advance 20] [--steps 20] [--windows 3]
                               [--arms off fusion noise_fusion noise_filter_fusion] [--parent-root DIR] [--no-kernel]
                               [--fusion '{"trunc": 0.5}'] [--out profiles/tsdf.json]
Three measurements:
  kernel    a 320 x 320 x 40 volume (voxel 0.25: an 80 x 80 x 10 unit scene) and 256 x 456 frames of a slanted scene: the single
            form on 1 and on 4 frames, the batch form on 12 volumes x 4 and x 1 frames in ring slots of 12 cameras' rings, the
            extraction (count + scan + emit into a buffer of the right size) and the statistics, beside a plain device copy of the
            same volume, which is the traffic floor (the parent commit has nothing to compare with).  HIP events around `launches`
            back-to-back calls after `warmup` untimed ones -> microseconds per call (median, min and max of 5 such blocks).
  rollouts  `rollouts` lock-step rollouts (bench.py's scenes and network) advanced un-timed to step `advance`, then `windows` timed
            windows of `steps` steps each -> exploration steps per second per window: "parent" (everything off, the package of the
            tree at --parent-root, which is a checkout of the parent commit with its library built, in a fresh child process that
            runs first), and in this process "off" and "fusion" (the option's defaults).
  quality   the arms "noise_fusion" and "noise_filter_fusion" (DESIGN.md 4p's noise and filter specs, fusion at its defaults, built
            with recon_metrics on): after the windows, the reconstruction metrics of the raw cloud and of the fused cloud, means over
            the rollouts: observations on one spec and `rollouts` scenes, not a gate.  "perfect_fusion" (on request) is the same
            table with perfect depth: what the fused cloud scores with no noise to average.
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
ARMS = {"off": {}, "fusion": {"fusion": True}, "noise_fusion": {"depth_noise": NOISE, "fusion": True},
        "noise_filter_fusion": {"depth_noise": NOISE, "depth_filter": FILTER, "fusion": True}, "perfect_fusion": {"fusion": True}}
QUALITY_ARMS = ("noise_fusion", "noise_filter_fusion", "perfect_fusion")    # ("perfect_fusion": perfect depth; not in the default arms)


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
    from nextbestpath_amd.simulator.camera import Camera
    from nextbestpath_amd.utility import hipops, tsdf
    H, W, voxel, trunc, max_depth = 256, 456, 0.25, 1.0, 70.0
    lo, dims = [-40.0, -5.0, -40.0], (320, 40, 320)     # x and z are the floor plan (320 voxels each), y the height (40)
    g = torch.Generator().manual_seed(1)
    col, row = torch.arange(W, dtype=torch.float32)[None, :], torch.arange(H, dtype=torch.float32)[:, None]
    rings = (8.0 + 12.0 * col / W + 0.01 * row)[None, None] + 4.0 * torch.rand(12, 16, 1, 1, generator=g)
    rings = rings.expand(12, 16, H, W).contiguous()
    rings[torch.rand(12, 16, H, W, generator=g) < 0.1] = -1.0
    rings = rings.to(dev)
    hw4 = H * W * 4
    # cameras on the floor plan, one heading each, as a rollout's lattice poses are
    cams = np.stack([[Camera.cam12_of_pose(None, np.array([-30.0 + 5.0 * r, 0.0, -20.0 + 3.0 * r + 0.5 * f, 0.0, 45.0 * ((r + f) % 8)],
                                                           np.float32)) for f in range(4)] for r in range(12)]).astype(np.float32)
    vols = [torch.zeros(*dims, 2, dtype=torch.int32, device=dev) for _ in range(12)]
    copy = torch.empty_like(vols[0])
    nbytes = vols[0].numel() * 4

    def slots(r, n):
        return [rings[r].data_ptr() + k * hw4 for k in range(4, 4 + n)]
    res = {"image": [H, W], "volume": list(dims), "volume_bytes": nbytes, "voxel": voxel, "trunc": trunc}
    res["device_copy_of_one_volume_us"] = event_us(lambda: copy.copy_(vols[0]), a.launches, a.warmup)
    for n in (1, 4):
        res[f"single_{n}_frames_us"] = event_us(lambda: hipops.tsdf_integrate(vols[0], lo, voxel, rings[0, 4:4 + n], cams[0, :n], trunc, max_depth),
                                                a.launches, a.warmup)
        items = [(vols[r], lo, voxel, trunc, max_depth, slots(r, n), cams[r, :n]) for r in range(12)]
        res[f"batch_12x{n}_frames_us"] = event_us(lambda: hipops.tsdf_integrate_batch(items, H, W), a.launches, a.warmup)
    vols[0].zero_()                                     # (the timed calls above added hundreds of observations: a fresh volume)
    for r in range(12):
        hipops.tsdf_integrate(vols[0], lo, voxel, rings[r, 4:8], cams[r], trunc, max_depth)
    pts, total = hipops.tsdf_extract(vols[0], lo, voxel, 1)
    st = hipops.tsdf_stats(vols[0], 1).tolist()
    host = vols[0].cpu().numpy()
    res["volume_after_48_frames"] = {"points": int(total.item()), "observed_voxels": st[0], "usable_voxels": st[1],
                                     "updated_share_of_voxels": round(st[0] / (dims[0] * dims[1] * dims[2]), 4),
                                     "equals_definition_stats": tsdf.stats(host, 1) == {"observed_voxels": st[0], "usable_voxels": st[1]}}
    out = torch.empty(max(pts.shape[0], 1), 3, dtype=torch.float32, device=dev)
    res["extract_us"] = event_us(lambda: hipops.tsdf_extract(vols[0], lo, voxel, 1, out=out), a.launches, a.warmup)
    res["stats_us"] = event_us(lambda: hipops.tsdf_stats(vols[0], 1), a.launches, a.warmup)
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
    tmp = tempfile.mkdtemp(prefix="nbp_bench_tsdf_")
    options = dict(options)
    rollout_kw = {"fusion": options.pop("fusion")} if "fusion" in options else {}      # (off passes nothing: the arm also runs on the parent)
    if quality:
        rollout_kw["recon_metrics"] = True
    ros = []
    for k in range(a.rollouts):
        name = f"maze{k}"
        make_maze_scene(os.path.join(tmp, name), seed=100 + k, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=0, **options)
        ros.append(tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=8 + k, **rollout_kw))
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
        if rollout_kw.get("fusion"):
            res["volume"] = list(ros[0].fusion.dims)
        if quality:
            def mean(vals):
                vals = [v for v in vals if v is not None]
                return None if not vals else round(float(np.mean(vals)), 5)

            def table(blocks):
                return {"accuracy_mean": mean(r["accuracy_mean"] for r in blocks), "completeness_mean": mean(r["completeness_mean"] for r in blocks),
                        "fscore": {str(t["threshold"]): mean(r["thresholds"][i]["fscore"] for r in blocks)
                                   for i, t in enumerate(blocks[0]["thresholds"])},
                        "precision": {str(t["threshold"]): mean(r["thresholds"][i]["precision"] for r in blocks)
                                      for i, t in enumerate(blocks[0]["thresholds"])},
                        "recall": {str(t["threshold"]): mean(r["thresholds"][i]["recall"] for r in blocks)
                                   for i, t in enumerate(blocks[0]["thresholds"])},
                        "n_points": mean(r["n_points"] for r in blocks)}
            t0 = time.perf_counter()
            fused = [r.fusion_metrics() for r in ros]
            t_fused = time.perf_counter() - t0
            res["quality"] = {"raw_cloud": table([r.reconstruction_metrics() for r in ros]), "fused_cloud": table(fused),
                              "usable_voxels": mean(f["usable_voxels"] for f in fused), "observed_voxels": mean(f["observed_voxels"] for f in fused),
                              "frames": fused[0]["frames"], "fusion_metrics_s_per_rollout": round(t_fused / len(ros), 4)}
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
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--advance", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--arms", nargs="*", default=[k for k in ARMS if k != "perfect_fusion"], choices=list(ARMS))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: adds the arm 'parent'")
    ap.add_argument("--root", default=None, help="import the package from this tree (what the 'parent' arm's child process does)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--fusion", default=None, help="the fusion option of the arms that have it on, as JSON (default: true = the defaults)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fusion = True if a.fusion is None else json.loads(a.fusion)
    for options in ARMS.values():
        if "fusion" in options:
            options["fusion"] = fusion
    res = {"bench": "tsdf", "noise": NOISE, "filter": FILTER, "fusion": fusion}
    if a.rollouts > 0 and a.arms:
        res["rollouts"] = {"rollouts": a.rollouts, "window": [a.advance, a.steps, a.windows]}
    if a.parent_root and "rollouts" in res:             # first, before this process opens the GPU: one process on it at a time
        res["rollouts"]["parent"] = parent_arm(a)
    assert torch.cuda.is_available(), "bench_tsdf measures on the GPU only"
    dev = torch.device("cuda")
    if not a.no_kernel:
        res["kernel"] = bench_kernel(a, dev)
    if a.rollouts > 0:
        for arm in a.arms:
            res["rollouts"][arm] = bench_rollouts(a, dev, ARMS[arm], quality=arm in QUALITY_ARMS)
            print(json.dumps({arm: res["rollouts"][arm]}), flush=True)      # (a long run shows its arms as they finish)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
