#!/usr/bin/env python
"""The compact replay record (csrc/nbp_replay.hip; nextbestpath_amd/utility/replay_codec.py) on real records: what it saves and
what it costs.

  1. Records are collected (reference format, K = 4 lock-step) from scenes of tools/make_synthetic_dataset.py's recipe; their
     planes give bytes per record in both formats and the width histogram per channel.
  2. hipops.replay_encode and hipops.replay_decode of n in {1, 16, 32} of those records at S = 256, beside a device-to-device copy
     of the same raw planes (n 6 S^2 floats read and written): HIP events around each call after warm-up, the three alternating in
     one process; the ratio to the copy is reported per n.

    python tools/bench_replay.py [--scenes 4] [--poses 60] [--launches 50] [--out profiles/r10/replay_kernels.json]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextbestpath_amd.utility import hipops, nbp_utils as nu, replay_codec  # noqa: E402


def collect(n_scenes, n_poses):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    net = net.cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(n_scenes):       # make_synthetic_dataset.py's default recipe
            make_maze_scene(os.path.join(tmp, "scenes", f"maze_{i:03d}"), seed=i, cells=10, size=6.0, height=1.2, tess=0.25,
                            hull="shell")
        env = nu.LogEnv(os.path.join(tmp, "db"))
        with torch.no_grad():
            nu.trajectory_collection(params, 1, sc.SceneDataset(os.path.join(tmp, "scenes")), env, (256, 256), (64, 64), (-40, 40),
                                     net, [], None, torch.device("cuda"), n_poses=n_poses, n_gt_points=20000, rollouts_per_gpu=4)
        return [v for _, v in env.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--poses", type=int, default=60)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles/r10/replay_kernels.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_replay.py measures on the GPU"
    values = collect(a.scenes, a.poses)
    assert len(values) >= 32, f"only {len(values)} records collected: raise --scenes / --poses"
    recs = [nu.unpack_record(v) for v in values]
    hist = [{0: 0, 1: 0, 2: 0, 4: 0} for _ in range(6)]
    nnz = np.zeros(6)
    compact_bytes = []
    for d, v in zip(recs, values):
        comp = nu.pack_record(d, "compact")
        compact_bytes.append(len(comp))
        chans = replay_codec.parse_header(nu.unpack_record(comp, keep_compact=True)["nbpc"])[2]
        for c, (n, w) in enumerate(chans):
            hist[c][w] += 1
            nnz[c] += n
    S = recs[0]["current_model_input"].shape[-1]
    ref_bytes = [len(v) for v in values]
    planes = np.stack([np.concatenate([d["current_model_input"][0], d["current_gt_2d_layout"][0]]) for d in recs[:32]])
    dev = torch.device("cuda")

    def timed(fns):
        """{name: fn} -> {name: median / min / max us}: the candidates alternate inside every round"""
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(a.launches):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) * 1e3)
        return {k: {"median_us": round(sorted(v)[len(v) // 2], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                for k, v in ms.items()}

    kernels = {}
    for n in (1, 16, 32):
        rec = torch.from_numpy(planes[:n]).to(dev)
        dst = torch.empty_like(rec)
        arena = hipops.replay_encode(rec)
        stride = arena.shape[1]
        used = [replay_codec.used_bytes(row) for row in arena.cpu().numpy()]
        # the decoder's input as the trainer stages it: the streams back to back, each padded to 16 bytes
        offsets = np.concatenate([[0], np.cumsum([(u + 15) & ~15 for u in used])]).tolist()
        packed = torch.cat([arena[r, :offsets[r + 1] - offsets[r]] for r in range(n)]).contiguous()
        x, gt = torch.empty(n, 5, S, S, device=dev), torch.empty(n, 1, S, S, device=dev)
        res = timed({"copy_d2d": lambda: dst.copy_(rec),
                     "encode": lambda: hipops.replay_encode(rec, arena),
                     "decode": lambda: hipops.replay_decode(packed, offsets[:-1], S, out=(x, gt))})
        assert torch.equal(x.view(torch.int32), rec[:, :5].contiguous().view(torch.int32))
        raw = n * 6 * S * S * 4
        for k in ("encode", "decode"):
            res[k]["x_copy"] = round(res[k]["median_us"] / res["copy_d2d"]["median_us"], 3)
        res["raw_bytes"], res["stream_bytes"], res["arena_stride"] = raw, int(sum(used)), int(stride)
        kernels[str(n)] = res
    out = {"metric": "compact replay record: size and kernel time", "size": S, "records": len(values),
           "collected_from": f"{a.scenes} synthetic mazes x {a.poses} poses, K = 4",
           "bytes_per_record": {"reference": round(float(np.mean(ref_bytes)), 1), "compact": round(float(np.mean(compact_bytes)), 1),
                                "compact_max": int(max(compact_bytes)),
                                "ratio": round(float(np.sum(ref_bytes) / np.sum(compact_bytes)), 2)},
           "width_histogram_per_channel": [{str(w): c for w, c in h.items()} for h in hist],
           "mean_nonzero_fraction_per_channel": [round(float(v / len(values) / (S * S)), 4) for v in nnz],
           "timer": "HIP events around each call, candidates alternating, after warm-up", "launches": a.launches,
           "kernels": kernels, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
