"""Trajectory collection, serial against lock-step: N synthetic mazes (make_maze_scene) collected with rollouts_per_gpu = 1 and
K (default 16), alternating in one process after a warm-up run of each.  Reports poses/s, records/s and the lock-step's stage split
(scene setup, GPU step, host search, record packing, store puts); writes profiles/r07/collect_lockstep.json.

    python tools/bench_collect.py [--scenes 16] [--k 16] [--poses 100] [--reps 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.simulator import scene as sc  # noqa: E402
from nextbestpath_amd.simulator.mesh import make_maze_scene  # noqa: E402
from nextbestpath_amd.testers import nbp_planning as tp  # noqa: E402
from nextbestpath_amd.utility import nbp_utils as nu  # noqa: E402
from nextbestpath_amd.utility.synthetic import make_explorer_state_dict  # noqa: E402


def run(params, ds, net, K, n_poses, tmp, tag, replay_format="reference"):
    env = nu.open_experience_db(os.path.join(tmp, tag))
    timing = {}
    counted = []
    orig = nu.CollectionRollout._observed

    def observed(self, pose_i, cov):               # counts the poses every rollout observes (both paths call this host half)
        counted.append(1)
        return orig(self, pose_i, cov)

    nu.CollectionRollout._observed = observed
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = nu.trajectory_collection(params, 1, ds, env, (256, 256), (64, 64), (-40, 40), net, [], None, torch.device("cuda"),
                                     n_poses=n_poses, n_gt_points=50000, rollouts_per_gpu=K, timing=timing,
                                     replay_format=replay_format)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        nu.CollectionRollout._observed = orig
    entries = env.entries()
    value_bytes = sum(len(v) for _, v in env.items())
    env.close()
    out = {"replay_format": replay_format, "value_bytes": value_bytes, "K": K, "seconds": round(dt, 3), "poses": len(counted), "records": n, "entries": entries,
           "poses_per_s": round(len(counted) / dt, 1), "records_per_s": round(n / dt, 1)}
    if timing:
        out["stages_s"] = {k: round(v, 3) for k, v in timing.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles/r07/collect_lockstep.json"))
    ap.add_argument("--replay-format", choices=nu.REPLAY_FORMATS, default="reference",
                    help="the records' format (nbp_utils.pack_record): the reference's, or the compact one encoded on the device")
    a = ap.parse_args()
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    net = net.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(a.scenes):
            make_maze_scene(os.path.join(tmp, "scenes", f"maze_{i:02d}"), seed=10 + i, cells=6, size=4.8, height=1.2, tess=0.4,
                            hull="shell")
        ds = sc.SceneDataset(os.path.join(tmp, "scenes"))
        runs = []
        with torch.no_grad():
            for K in (1, a.k):                                     # warm-up of each setting
                run(params, ds, net, K, a.poses, tmp, f"warm_k{K}", a.replay_format)
            for r in range(a.reps):
                for K in (1, a.k):
                    res = run(params, ds, net, K, a.poses, tmp, f"r{r}_k{K}", a.replay_format)
                    print(json.dumps(res), flush=True)
                    runs.append(res)
    best = {K: max((x for x in runs if x["K"] == K), key=lambda x: x["poses_per_s"]) for K in (1, a.k)}
    summary = {"replay_format": a.replay_format, "scenes": a.scenes, "n_poses": a.poses, "K": a.k, "runs": runs,
               "poses_per_s": {str(K): v["poses_per_s"] for K, v in best.items()},
               "records_per_s": {str(K): v["records_per_s"] for K, v in best.items()},
               "speedup_poses": round(best[a.k]["poses_per_s"] / best[1]["poses_per_s"], 2),
               "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(summary, fh, indent=1)
    print(json.dumps({k: summary[k] for k in ("poses_per_s", "records_per_s", "speedup_poses")}))


if __name__ == "__main__":
    main()
