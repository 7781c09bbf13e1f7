#!/usr/bin/env python
"""Cost and effect of the cloud-to-mesh accuracy metrics (hipops.MeshPlan / SurfaceMetrics, csrc/nbp_surface.hip).
    python tools/bench_surface.py [--launches 20] [--warmup 3] [--rollouts 48] [--steps 80] [--arms perfect noise noise_filter]
                                  [--surface '{"cell": 0.5}'] [--out profiles/surface.json]
Reports, gates nothing.  Per arm, `rollouts` lock-step rollouts (bench.py's scenes and network) run `steps` steps with fusion,
recon_metrics and surface_metrics on; then
  quality   DESIGN.md 4q's table again, with the yardstick that has no floor: accuracy_mean / accuracy_rmse / precision per
            threshold against the MESH, raw cloud and fused cloud, beside accuracy_mean against the GT sample (recon_metrics), means
            over the rollouts.  Arms: "perfect" (perfect depth), "noise", "noise_filter" (4p's noise and filter specs).
  launches  on the first arm's first rollout, its final cloud and its mesh: the plan build (count, scan, read-back, fill: wall clock,
            it synchronises), the query launch, the statistics, beside NNPlan.dist2 of the same cloud against the GT sample -- the
            launch it stands next to (the parent commit has nothing else to compare with).  HIP events around `launches` back-to-back
            calls after `warmup` untimed ones -> microseconds per call (median, min and max of 5 such blocks).
  size      entries per triangle, and triangle evaluations per query: from the plan's per-cell counts read back and the shell each
            query's walk ends with (the first r >= r0 with d2 <= fl(r cell)^2, or R, or the one that covers the grid).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

NOISE = {"sigma_base": 0.01, "sigma_quad": 0.001, "dropout": 0.02, "edge_threshold": 2.0}
FILTER = {"radius": 1, "range_base": 0.03, "range_quad": 0.003, "min_support": 2, "fill_support": 6}
ARMS = {"perfect": {}, "noise": {"depth_noise": NOISE}, "noise_filter": {"depth_noise": NOISE, "depth_filter": FILTER}}


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


def evaluations_per_query(sm_dev, cloud, d2):
    """Triangle evaluations of each query's walk -> float64 [n], from the plan's per-cell counts and the distances it produced."""
    from nextbestpath_amd.utility import surface_metrics as sm
    plan = sm_dev.plan
    lo, hi = np.asarray(sm_dev.box[0], np.float32), np.asarray(sm_dev.box[1], np.float32)
    n, inv = sm.grid_dims(lo, hi, plan.cell)
    ncell = int(np.prod(n))
    off = -plan.plan.data_ptr() % 256
    start = plan.plan[off:off + 4 * (ncell + 1)].view(torch.int32).cpu().numpy().astype(np.int64)
    count = np.diff(start).reshape(n)
    integral = np.zeros(tuple(n + 1), np.int64)                     # integral[i, j, k] = the entries of cells [0, i) x [0, j) x [0, k)
    integral[1:, 1:, 1:] = count.cumsum(0).cumsum(1).cumsum(2)
    w, R = np.float32(plan.cell), int(np.ceil(sm_dev.cap / plan.cell))
    c = np.floor((cloud - lo) * inv)
    ok = np.all(np.isfinite(c) & (c >= -R) & (c <= (n - 1 + R)), axis=1)
    c = np.where(ok[:, None], c, 0).astype(np.int64)
    r0 = np.maximum(np.maximum(-c, c - (n - 1)).max(1), 0)
    covers = np.maximum(c, n - 1 - c).max(1)                        # the shell that reaches every cell of the grid
    rw = (np.arange(R + 1, dtype=np.float32) * w) ** 2
    r_stop = np.searchsorted(rw, d2, side="left")                   # the first r with d2 <= fl(r w)^2
    r_end = np.minimum(np.minimum(np.maximum(r_stop, r0), R), np.maximum(covers, r0))
    a0, a1 = np.clip(c - r_end[:, None], 0, n), np.clip(c + r_end[:, None] + 1, 0, n)
    box = 0
    for sx, ix in ((1, a1[:, 0]), (-1, a0[:, 0])):
        for sy, iy in ((1, a1[:, 1]), (-1, a0[:, 1])):
            for sz, iz in ((1, a1[:, 2]), (-1, a0[:, 2])):
                box = box + sx * sy * sz * integral[ix, iy, iz]
    return np.where(ok, box, 0).astype(np.float64)


def bench_launches(a, dev, ro):
    from nextbestpath_amd.utility import hipops
    n = int(ro.st.cloud_count.item())
    cloud, mesh, sm_dev = ro.st.cloud[:n].contiguous(), ro.mesh, ro.surface
    res = {"cloud_points": n, "gt_points": int(ro.gt.shape[0]), "mesh": sm_dev.mesh_block(), "cell": sm_dev.cell, "cap": sm_dev.cap}
    builds = []
    for _ in range(a.warmup + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hipops.MeshPlan(mesh.verts, mesh.faces, sm_dev.box, sm_dev.cell)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e6)
    builds = builds[a.warmup:]
    res["mesh_plan_build_wall_us"] = {"median": round(float(np.median(builds)), 1), "min": round(min(builds), 1), "max": round(max(builds), 1)}
    out = torch.empty(n, dtype=torch.float32, device=dev)
    res["mesh_dist2_us"] = event_us(lambda: sm_dev.plan.dist2(cloud, sm_dev.cap, out=out), a.launches, a.warmup)
    d2 = out.cpu().numpy()
    res["stats_us"] = event_us(lambda: hipops.recon_stats(out, sm_dev.thresholds), a.launches, a.warmup)
    res["surface_evaluate_us"] = event_us(lambda: sm_dev.evaluate(cloud), a.launches, a.warmup)
    out_nn = torch.empty(n, dtype=torch.float32, device=dev)
    res["nn_dist2_against_the_gt_sample_us"] = event_us(lambda: ro.recon.plan.dist2(cloud, ro.recon.cap, out=out_nn), a.launches, a.warmup)
    ev = evaluations_per_query(sm_dev, cloud.cpu().numpy(), d2)
    res["size"] = {"entries_per_triangle": round(sm_dev.plan.entries / max(sm_dev.plan.faces_used, 1), 3),
                   "evaluations_per_query": {"mean": round(float(ev.mean()), 1), "median": float(np.median(ev)), "max": float(ev.max())},
                   "share_of_queries_at_the_cap": round(float((d2 >= np.float32(sm_dev.cap) ** 2).mean()), 5)}
    return res


def bench_arm(a, dev, options, surface, launches):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9), strict=True)
    net = net.to(dev).eval()
    tmp = tempfile.mkdtemp(prefix="nbp_bench_surface_")
    ros = []
    t0 = time.perf_counter()
    for k in range(a.rollouts):
        name = f"maze{k}"
        make_maze_scene(os.path.join(tmp, name), seed=100 + k, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=0, **options)
        ros.append(tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=8 + k, recon_metrics=True,
                              fusion=True, surface_metrics=surface))
    torch.cuda.synchronize()
    res = {"setup_s": round(time.perf_counter() - t0, 2)}
    multi = tp.MultiRollout(ros, net, dev)
    with torch.no_grad():
        for _ in range(a.steps):
            multi.step()
        multi.flush()
        torch.cuda.synchronize()

        def mean(vals):
            vals = [v for v in vals if v is not None]
            return None if not vals else round(float(np.mean(vals)), 5)

        def table(blocks):
            return {"accuracy_mean": mean(b["accuracy_mean"] for b in blocks), "accuracy_rmse": mean(b["accuracy_rmse"] for b in blocks),
                    "precision": {str(t["threshold"]): mean(b["thresholds"][i]["precision"] for b in blocks)
                                  for i, t in enumerate(blocks[0]["thresholds"])},
                    "n_points": mean(b["n_points"] for b in blocks)}
        t0 = time.perf_counter()
        blocks = [r.surface_metrics() for r in ros]
        t_surface = time.perf_counter() - t0
        res["against_the_mesh"] = {"raw_cloud": table([b["cloud"] for b in blocks]), "fused_cloud": table([b["fused"] for b in blocks]),
                                   "surface_metrics_s_per_rollout": round(t_surface / len(ros), 4)}
        res["against_the_gt_sample"] = {"raw_cloud_accuracy_mean": mean(r.reconstruction_metrics()["accuracy_mean"] for r in ros),
                                        "fused_cloud_accuracy_mean": mean(r.fusion_metrics()["accuracy_mean"] for r in ros)}
        res["mesh"] = {k: mean(b["mesh"][k] for b in blocks) for k in ("faces", "faces_used", "entries")}
        res["mean_final_coverage"] = round(float(np.mean([r.coverage_evolution(a.steps)[-1] for r in ros])), 4)
        if launches:
            res["launches"] = bench_launches(a, dev, ros[0])
    del multi, ros
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--arms", nargs="*", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--surface", default=None, help="the surface_metrics option as JSON (default: true = the defaults)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    surface = True if a.surface is None else json.loads(a.surface)
    assert torch.cuda.is_available(), "bench_surface measures on the GPU only"
    dev = torch.device("cuda")
    res = {"bench": "surface", "noise": NOISE, "filter": FILTER, "surface_metrics": surface, "rollouts": a.rollouts, "steps": a.steps, "arms": {}}
    for i, arm in enumerate(a.arms):
        res["arms"][arm] = bench_arm(a, dev, ARMS[arm], surface, launches=i == 0)
        print(json.dumps({arm: res["arms"][arm]}), flush=True)      # (a long run shows its arms as they finish)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
