#!/usr/bin/env python
"""Cost and effect of the fused mesh (hipops.tsdf_mesh / FusedMeshMetrics, csrc/nbp_tsdf_mesh.hip).
    python tools/bench_tsdf_mesh.py [--launches 100] [--warmup 5] [--runs 3] [--rollouts 48] [--steps 80]
                                    [--arms perfect noise noise_filter] [--no-kernel] [--ply PATH] [--out profiles/tsdf_mesh.json]
Reports, gates nothing (the parent commit has nothing to compare with).
  kernel    DESIGN.md 4q's protocol and volume: 320 x 40 x 320 voxels of 0.25 with 48 frames of tools/bench_tsdf.py's slanted scene
            integrated.  HIP events around `launches` back-to-back calls after `warmup` untimed ones -> microseconds per call (median,
            min and max of 5 such blocks), `runs` times in this one session: the mesh's counting form (count + scan), its sized form
            (count, scan, vertices, faces with their squared areas, into buffers of the right size) and that form's parts (vertices
            alone; without the areas; the areas with no vertex buffer to read back, every vertex made again), beside a plain device copy of the
            volume -- the traffic floor -- and tsdf_extract (count, scan, emit) of the same volume.  FusedMeshMetrics.evaluate (the
            mesh, a MeshPlan over it, GT -> mesh distances of 100 000 points of a box around the volume, the statistics; it reads
            counts back, so wall clock, median of 5) against that box.
  quality   per arm of DESIGN.md 4r ("perfect" depth, "noise", "noise_filter": 4p's specs), `rollouts` lock-step rollouts (bench.py's
            scenes and network) run `steps` steps with recon_metrics and fusion with `mesh` on: completeness GT -> fused MESH
            (fused_mesh_metrics) beside completeness GT -> fused CLOUD (fusion_metrics, recon_metrics' nearest neighbour), from the
            same volumes, means over the rollouts; the mesh's counts, area and vertex accuracy beside them.
  --ply     writes the fused mesh of one frontier-policy rollout (`steps` steps) on a synthetic maze as a binary PLY; needs no
            checkpoint.
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
FUSION = {"mesh": True}


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


def wall_us(fn, warmup, blocks=5):
    out = []
    for k in range(warmup + blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    out = out[warmup:]
    return {"median": round(float(np.median(out)), 1), "min": round(min(out), 1), "max": round(max(out), 1)}


def box_mesh(lo, hi, n, seed=0):
    """An axis-aligned box (12 triangles) and n points on its faces: the GT of the kernel section's FusedMeshMetrics."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts = np.array([[(lo, hi)[(m >> d) & 1][d] for d in range(3)] for m in range(8)], np.float32)
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                      [1, 3, 5], [3, 7, 5]], np.int32)
    rng = np.random.default_rng(seed)
    f, u, v = rng.integers(0, 12, n), rng.random(n), rng.random(n)
    swap = u + v > 1
    u[swap], v[swap] = 1 - u[swap], 1 - v[swap]
    a, b, c = (verts[faces[f, k]].astype(np.float64) for k in range(3))
    return verts, faces, (a + u[:, None] * (b - a) + v[:, None] * (c - a)).astype(np.float32)


def bench_kernel(a, dev):
    from types import SimpleNamespace
    from nextbestpath_amd.simulator.camera import Camera
    from nextbestpath_amd.utility import hipops, tsdf
    H, W, voxel, trunc, max_depth = 256, 456, 0.25, 1.0, 70.0
    lo, dims = [-40.0, -5.0, -40.0], (320, 40, 320)     # tools/bench_tsdf.py's volume and frames
    g = torch.Generator().manual_seed(1)
    col, row = torch.arange(W, dtype=torch.float32)[None, :], torch.arange(H, dtype=torch.float32)[:, None]
    rings = (8.0 + 12.0 * col / W + 0.01 * row)[None, None] + 4.0 * torch.rand(12, 16, 1, 1, generator=g)
    rings = rings.expand(12, 16, H, W).contiguous()
    rings[torch.rand(12, 16, H, W, generator=g) < 0.1] = -1.0
    rings = rings.to(dev)
    cams = np.stack([[Camera.cam12_of_pose(None, np.array([-30.0 + 5.0 * r, 0.0, -20.0 + 3.0 * r + 0.5 * f, 0.0, 45.0 * ((r + f) % 8)],
                                                           np.float32)) for f in range(4)] for r in range(12)]).astype(np.float32)
    spec = tsdf.resolved_options(tsdf.option_spec({"voxel": voxel, "trunc": trunc, "mesh": True}), max_depth)
    tv = hipops.TSDFVolume(([lo[0] + trunc, lo[1] + trunc, lo[2] + trunc], [lo[0] + 80.0 - trunc, lo[1] + 10.0 - trunc, lo[2] + 80.0 - trunc]),
                           spec, dev)
    assert tv.dims == dims and tv.lo == lo
    for r in range(12):
        tv.integrate(rings[r, 4:8], cams[r])
    vol = tv.vol
    copy = torch.empty_like(vol)
    pts, total = hipops.tsdf_extract(vol, lo, voxel, 1)
    verts, faces, totals = hipops.tsdf_mesh(vol, lo, voxel, 1)
    st = hipops.tsdf_stats(vol, 1).tolist()
    nv, nf = (int(v) for v in totals.tolist())
    res = {"volume": list(dims), "volume_bytes": vol.numel() * 4, "voxel": voxel, "frames": tv.frames, "points": int(total.item()),
           "vertices": nv, "faces": nf, "observed_voxels": st[0], "usable_voxels": st[1], "runs": []}
    out_pts = torch.empty(max(pts.shape[0], 1), 3, dtype=torch.float32, device=dev)
    verts, faces = torch.empty(max(nv, 1), 3, dtype=torch.float32, device=dev), torch.empty(max(nf, 1), 3, dtype=torch.int32, device=dev)
    area2 = torch.empty(max(nf, 1), dtype=torch.float32, device=dev)
    none = torch.empty(0, 3, dtype=torch.float32, device=dev)
    blo, bhi = np.array(lo) + 2.0, np.array(lo) + np.array([78.0, 8.0, 78.0])
    gv, gf, gt = box_mesh(blo, bhi, 100_000)
    gt_mesh = SimpleNamespace(verts=torch.from_numpy(gv).to(dev), faces=torch.from_numpy(gf).to(dev), verts_host=gv)
    fm = hipops.FusedMeshMetrics(torch.from_numpy(gt).to(dev), hipops.SurfaceMetrics(gt_mesh))
    for _ in range(a.runs):
        run = {"device_copy_of_the_volume_us": event_us(lambda: copy.copy_(vol), a.launches, a.warmup),
               "extract_us": event_us(lambda: hipops.tsdf_extract(vol, lo, voxel, 1, out=out_pts), a.launches, a.warmup),
               "mesh_count_us": event_us(lambda: hipops.tsdf_mesh(vol, lo, voxel, 1, verts_out=none), a.launches, a.warmup),
               "mesh_vertices_only_us": event_us(lambda: hipops.tsdf_mesh(vol, lo, voxel, 1, verts_out=verts), a.launches, a.warmup),
               "mesh_without_areas_us": event_us(lambda: hipops.tsdf_mesh(vol, lo, voxel, 1, verts, faces), a.launches, a.warmup),
               "mesh_sized_us": event_us(lambda: hipops.tsdf_mesh(vol, lo, voxel, 1, verts, faces, area2), a.launches, a.warmup),
               "mesh_areas_without_a_vertex_buffer_us": event_us(lambda: hipops.tsdf_mesh(vol, lo, voxel, 1, None, faces, area2), a.launches,
                                                                 a.warmup),
               "fused_mesh_metrics_wall_us": wall_us(lambda: fm.evaluate(tv), 2)}
        res["runs"].append(run)
        print(json.dumps({"kernel_run": run}), flush=True)
    res["fused_mesh_metrics_block"] = fm.summary()
    return res


def make_rollouts(a, dev, options, policy=None, n=None):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    if policy is None:
        net = NBP()
        net.load_state_dict(make_explorer_state_dict(9), strict=True)
        net = net.to(dev).eval()
    else:
        from nextbestpath_amd.testers.frontier_policy import make_policy
        net = make_policy(policy)
    tmp = tempfile.mkdtemp(prefix="nbp_bench_tsdf_mesh_")
    ros = []
    for k in range(a.rollouts if n is None else n):
        name = f"maze{k}"
        make_maze_scene(os.path.join(tmp, name), seed=100 + k, cells=10, size=6.0, height=1.2, tess=0.25)
        ds = sc.SceneDataset(tmp, [name])
        settings = sc.Settings(ds[0]["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(tmp, name, ds[0]["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=0)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=0, **options)
        ros.append(tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=8 + k, recon_metrics=True,
                              fusion=FUSION))
    multi = tp.MultiRollout(ros, net, dev)
    with torch.no_grad():
        for _ in range(a.steps):
            multi.step()
        multi.flush()
    torch.cuda.synchronize()
    return ros, multi


def bench_arm(a, dev, options):
    ros, multi = make_rollouts(a, dev, options)

    def mean(vals):
        vals = [v for v in vals if v is not None]
        return None if not vals else round(float(np.mean(vals)), 5)
    with torch.no_grad():
        t0 = time.perf_counter()
        meshes = [r.fused_mesh_metrics() for r in ros]
        t_mesh = time.perf_counter() - t0
        clouds = [r.fusion_metrics() for r in ros]
    comp = [m["completeness"] for m in meshes]
    res = {"against_the_fused_mesh": {"completeness_mean": mean(c["completeness_mean"] for c in comp),
                                      "completeness_rmse": mean(c["completeness_rmse"] for c in comp),
                                      "recall": {str(t["threshold"]): mean(c["thresholds"][i]["recall"] for c in comp)
                                                 for i, t in enumerate(comp[0]["thresholds"])}},
           "against_the_fused_cloud": {"completeness_mean": mean(c["completeness_mean"] for c in clouds),
                                       "completeness_rmse": mean(c["completeness_rmse"] for c in clouds),
                                       "recall": {str(t["threshold"]): mean(c["thresholds"][i]["recall"] for c in clouds)
                                                  for i, t in enumerate(clouds[0]["thresholds"])},
                                       "n_points": mean(c["n_points"] for c in clouds)},
           "mesh": {k: mean(m[k] for m in meshes) for k in ("vertices", "faces", "quads", "crossings", "area")},
           "vertex_accuracy_mean_against_the_gt_mesh": mean(m["accuracy"]["accuracy_mean"] for m in meshes),
           "volume": list(ros[0].fusion.dims), "fused_mesh_metrics_s_per_rollout": round(t_mesh / len(ros), 4),
           "mean_final_coverage": round(float(np.mean([r.coverage_evolution(a.steps)[-1] for r in ros])), 4)}
    del multi, ros
    torch.cuda.empty_cache()
    return res


def write_ply(a, dev):
    from nextbestpath_amd.utility import tsdf_mesh
    ros, multi = make_rollouts(a, dev, {}, policy="frontier", n=1)
    verts, faces = ros[0].fused_mesh()
    os.makedirs(os.path.dirname(os.path.abspath(a.ply)), exist_ok=True)
    tsdf_mesh.write_ply(a.ply, verts.cpu().numpy(), faces.cpu().numpy())
    return {"path": a.ply, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "steps": a.steps, "policy": "frontier"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rollouts", type=int, default=48)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--arms", nargs="*", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--ply", default=None, help="write the fused mesh of one frontier-policy rollout here (binary PLY)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_mesh measures on the GPU only"
    dev = torch.device("cuda")
    res = {"bench": "tsdf_mesh", "noise": NOISE, "filter": FILTER, "fusion": FUSION, "rollouts": a.rollouts, "steps": a.steps}
    if a.ply:
        res["ply"] = write_ply(a, dev)
    if not a.no_kernel:
        res["kernel"] = bench_kernel(a, dev)
    if a.rollouts > 0 and a.arms:
        res["arms"] = {}
        for arm in a.arms:
            res["arms"][arm] = bench_arm(a, dev, ARMS[arm])
            print(json.dumps({arm: res["arms"][arm]}), flush=True)      # (a long run shows its arms as they finish)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
