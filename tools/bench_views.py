#!/usr/bin/env python
"""Time of the held-out view metrics (hipops.ViewMetrics, csrc/nbp_views.hip) over the cloud of a real rollout.
    python tools/bench_views.py [--poses 100] [--views 16] [--height 256 --width 456] [--launches 20] [--warmup 3] [--out FILE]
Inputs: the benchmark's maze (cells 10, size 6.0, seed 100), the default parameters (gathering_factor 0.05, 256 x 456 frames), one
rollout of `poses` steps with the synthetic explorer weights; its coloured cloud stays in the rollout's buffer with its length in
the device counter.  The evaluation poses are the option's own (view_metrics.choose_views from the rollout's start, seed 0).
Arms, each timed with HIP events around every call from an idle stream, `warmup` untimed calls first, all in this process; the
arms that are compared with each other (the two splat forms) alternate call by call:
    evaluate_r{0,1,2}       ViewMetrics.evaluate: the clear, the splat of the whole cloud (one launch per 8 views), the statistics
    splat_r{0,1,2}_precheck the splat alone (clear included), a plain load in front of every atomic
    splat_r{0,1,2}_atomic   ... every footprint pixel goes to the atomic
    stats                   resolve + classify + reduce alone (two launches: call time, mostly their latency)
    recon_evaluate          ReconMetrics.evaluate on the same cloud: the yardstick for an end-of-rollout metric
    gt_render               the choice of the poses and the mesh render of the views (once per rollout)
Prints one JSON line (and writes it to --out): per arm the median (min - max) in microseconds, the bytes the splat has to read
(12 B per point per chunk of 8 views) with the rate they imply, and view_completeness / hole / leak / floater / psnr per radius."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextbestpath_amd.utility import hipops  # noqa: E402
from nextbestpath_amd.utility import view_metrics as vm  # noqa: E402


def timed(fns, launches, warmup):
    """{name: fn} -> {name: [microseconds]}: the arms alternate call by call."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_views measures on the GPU only"
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    dev = torch.device("cuda")
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    tmp = tempfile.mkdtemp(prefix="nbp_bench_views_")
    make_maze_scene(os.path.join(tmp, "maze"), seed=100, cells=10, size=6.0, height=1.2, tess=0.25)
    ds = sc.SceneDataset(tmp, ["maze"])
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9), strict=True)
    net = net.to(dev).eval()
    spec = {"views": a.views}
    if a.height:
        spec["height"] = a.height
    if a.width:
        spec["width"] = a.width
    with torch.no_grad():
        ro = tp.build_rollout(params, net, ds, tp.list_runs(ds, params)[0], dev, seed=8, recon_metrics=True, view_metrics=spec)
        for _ in range(a.poses):
            ro.step()
        ro.finish()
    torch.cuda.synchronize()
    shutil.rmtree(tmp, ignore_errors=True)             # (the scene is on the device)
    st, cam = ro.st, ro.camera
    N = int(st.cloud_count.item())
    base = ro.views
    V, H, W = base.V, base.H, base.W
    rgb = st.cloud_rgb if cam.renders_colours else None
    res, quality = {}, {}
    objs = {r: hipops.ViewMetrics(None, base.cams, H, W, radius=r, depth_tolerance=base.depth_tolerance, z_far=base.z_far,
                                  ground_truth=(base.z_gt, base.rgb_gt)) for r in (0, 1, 2)}
    for r, obj in objs.items():
        res.update(timed({f"evaluate_r{r}": lambda obj=obj: obj.evaluate(st.cloud, rgb, st.cloud_count)}, a.launches, a.warmup))
        block = obj.summary()
        quality[f"r{r}"] = {k: block[k] for k in ("view_completeness", "hole", "leak", "floater", "depth_mae", "psnr")}
        keys = torch.empty_like(obj.keys)
        res.update(timed({f"splat_r{r}_precheck": lambda r=r, keys=keys: hipops.splat_cloud(st.cloud, base.cams, H, W, r, st.cloud_count,
                                                                                           base.z_far, keys, precheck=True),
                          f"splat_r{r}_atomic": lambda r=r, keys=keys: hipops.splat_cloud(st.cloud, base.cams, H, W, r, st.cloud_count,
                                                                                         base.z_far, keys, precheck=False)},
                         a.launches, a.warmup))
        assert torch.equal(keys, obj.keys)                 # (whichever form ran last: the same bits as the evaluation's)
    o1 = objs[1]
    res.update(timed({"stats": lambda: hipops.view_stats(o1.keys, rgb, o1.z_gt, o1.rgb_gt if rgb is not None else None,
                                                         o1.depth_tolerance, o1.z_far, st.cloud.shape[0])}, a.launches, a.warmup))
    res.update(timed({"recon_evaluate": lambda: ro.recon.evaluate(st.cloud, st.cloud_count)}, a.launches, a.warmup))
    res.update(timed({"gt_render": lambda: ro._build_views(ro.view_spec)}, max(3, a.launches // 4), 1))
    chunks = -(-V // 8)
    splat_bytes = 12 * N * chunks
    rates = {k: round(splat_bytes / (v["median_us"] * 1e-6) / 1e9, 1) for k, v in res.items() if k.startswith("splat_")}
    line = json.dumps({"metric": "held-out view metrics time at a rollout's end", "N": N, "capacity": st.cloud.shape[0], "poses": a.poses,
                       "views": V, "height": H, "width": W, "pixels_per_view": H * W, "launches": a.launches, "warmup": a.warmup,
                       "timer": "HIP events around each call from an idle stream; compared arms alternate call by call",
                       "splat_read_bytes": splat_bytes, "splat_read_GBps": rates, "results": res, "quality_by_radius": quality,
                       "options": dict(base.options), "raw_width": vm.RAW_WIDTH})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
