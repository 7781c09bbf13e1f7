#!/usr/bin/env python
"""Config 3 of BASELINE.json: NBP fwd + bwd + AdamW step, batch of 256x256 maps, fp32, 1 MI355X.
    python tools/bench_train.py [--batch 32] [--steps 5] [--size 256] [--precision fp32_split|fp16] [--augment P]
                                [--optimizer torch|hip] [--clip X] [--ema D] [--priority ALPHA]
Prints one JSON line: train maps/s, TFLOP/s against 546.9 GFLOP/map, and the torch-CPU baseline
(stock autograd on the same weights = the reference's arithmetic) on a bounded sample."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks import training as tr  # noqa: E402
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.trainers.train_nbp_model import _collate, make_optimizer, make_synthetic_experiences  # noqa: E402
from nextbestpath_amd.utility import augment, hipops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cpu-batch", type=int, default=2)
    ap.add_argument("--precision", choices=tr.TRAIN_PRECISIONS, default="fp32_split",
                    help="NBP.train_precision: the split path (default) or scaled fp16 mixed precision")
    ap.add_argument("--augment", type=float, default=0.0,
                    help="augment_probability: with P > 0 every step draws its op codes, remaps the targets on the host, copies the "
                         "codes to the device and moves the batch with hipops.augment_batch (the trainer's per-batch work)")
    ap.add_argument("--optimizer", choices=("torch", "hip"), default="torch",
                    help="make_optimizer's impl: torch's fused AdamW (default) or HipAdamW (csrc/nbp_optim.hip)")
    ap.add_argument("--clip", type=float, default=None,
                    help="grad_clip_norm X > 0: global-norm clipping inside HipAdamW.step() (needs --optimizer hip)")
    ap.add_argument("--ema", type=float, default=None,
                    help="ema_decay D in [0, 1): a WeightEMA of the network (csrc/nbp_ema.hip), updated behind every optimizer step")
    ap.add_argument("--replay-format", choices=("reference", "compact"), default=None,
                    help="with a format every step also runs the trainer's per-batch data path on records of that format: staged "
                         "collation (reference: the expanded maps; compact: the streams + one hipops.replay_decode launch).  "
                         "Default: the batch is collated once, outside the timed steps")
    ap.add_argument("--priority", type=float, default=None, metavar="ALPHA",
                    help="replay_priority_alpha: every step draws its batch from a ReplayPriorities over the records (with replacement), "
                         "copies the draw's weights to the device, runs the fused objective (tr.loss_weighted) instead of gather + "
                         "nbp.loss, and behind the optimizer step reads the per-sample terms back and updates the table (the trainer "
                         "does that once per 8 batches).  0 = uniform draws, unit weights")
    a = ap.parse_args()
    if a.replay_format and a.augment > 0:
        ap.error("--replay-format and --augment time different per-batch work: one at a time")
    if a.priority is not None and (a.replay_format or a.augment > 0):
        ap.error("--priority times its own per-batch work: not with --replay-format or --augment")
    dev = torch.device("cuda")
    torch.manual_seed(9)
    net = NBP().to(dev).train()
    net.train_precision = a.precision
    opt = make_optimizer(net, impl=a.optimizer, grad_clip_norm=a.clip)
    ema = None
    if a.ema is not None:
        from nextbestpath_amd.optim import WeightEMA
        ema = WeightEMA(net, a.ema)
    db = make_synthetic_experiences(a.batch, a.size, seed=3)
    xs, gt, coords, gains, bidx = _collate(db, dev)

    stager = None
    if a.replay_format:
        from nextbestpath_amd.trainers.train_nbp_model import _BatchStager, _await_batch, _collate_any
        from nextbestpath_amd.utility import nbp_utils as nu
        records = [nu.unpack_record(nu.pack_record(d, a.replay_format), keep_compact=True) for d in db]
        stager = _BatchStager(dev)

    prio = None
    if a.priority is not None:
        from nextbestpath_amd.utility import priority
        prio = priority.ReplayPriorities(a.priority)
        prio.begin(list(range(a.batch)))
        prio_rng = np.random.default_rng(5)
        first = torch.zeros(a.batch + 1, dtype=torch.int64)
        first[1:] = torch.bincount(bidx.cpu(), minlength=a.batch).cumsum(0)

    def prioritised_step():
        """A batch of drawn records: the planes by one device gather, the targets by index arithmetic on the host (the trainer collates
        the drawn records and stages them; the bytes that move to the device are the same weights, targets and op-free planes)."""
        idx, w = prio.draw(prio_rng, a.batch)
        idx_dev = torch.from_numpy(idx).pin_memory().to(dev, non_blocking=True)
        w_dev = torch.from_numpy(w.astype(np.float32)).pin_memory().to(dev, non_blocking=True)
        rows = np.concatenate([np.arange(int(first[i]), int(first[i + 1])) for i in idx])
        sizes = np.array([int(first[i + 1] - first[i]) for i in idx])
        rows_dev = torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True)
        bi = torch.from_numpy(np.repeat(np.arange(a.batch), sizes)).pin_memory().to(dev, non_blocking=True)
        o1, o2 = net(xs[idx_dev])
        loss, per_sample = tr.loss_weighted(net, o1, bi, coords[rows_dev], gains[rows_dev], o2, gt[idx_dev], w_dev)
        return loss, idx, per_sample

    aug_rng = random.Random(5)
    ops_dev = torch.zeros(a.batch, dtype=torch.int32, device=dev)

    def targets(records):
        """The sparse targets of remapped records on the device (pinned, asynchronous copies as the trainer's stager makes)."""
        cd = np.concatenate([d["target_value_map_pixel"] for d in records])
        gn = np.concatenate([d["actual_coverage_gain"] for d in records])
        bi = np.repeat(np.arange(len(records)), [len(d["target_value_map_pixel"]) for d in records])
        return [torch.from_numpy(v).pin_memory().to(dev, non_blocking=True) for v in (cd, gn, bi)]

    def step():
        drawn = None
        if prio is not None:
            loss, *drawn = prioritised_step()
        elif a.augment > 0:
            ops = augment.draw_ops(aug_rng, a.batch, a.augment)
            ops_dev.copy_(torch.from_numpy(ops).pin_memory(), non_blocking=True)
            cd, gn, bi = targets(augment.augment_records(db, ops, a.size // 4))
            xa, ga = hipops.augment_batch(xs, gt, ops_dev)
            o1, o2 = net(xa)
            loss = net.loss(tr.gather_values(o1, bi, cd), gn, o2, ga)
        elif stager is not None:
            tensors, ev = _collate_any(records, dev, stager)
            xb, gb, cd, gn, bi = _await_batch(tensors, ev, dev)
            o1, o2 = net(xb)
            loss = net.loss(tr.gather_values(o1, bi, cd), gn, o2, gb)
        else:
            o1, o2 = net(xs)
            loss = net.loss(tr.gather_values(o1, bidx, coords), gains, o2, gt)
        loss.backward()
        opt.step()
        if ema is not None:
            ema.update(opt)
        opt.zero_grad(set_to_none=True)
        if drawn is not None:
            terms = torch.cat([drawn[1].reshape(-1), net.log_vars.detach().double()]).cpu().numpy()
            prio.update(drawn[0].tolist(), priority.sample_loss(terms[:-2].reshape(-1, 3), a.size, terms[-2:]))
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    flop_map = 546.9e9 * (a.size / 256) ** 2
    # CPU baseline: torch autograd on the oracle network (bounded sample: cpu-batch maps, 1 step; --cpu-batch 0: none -- profiling runs,
    # whose copy counts would otherwise include the 327 device -> host copies of the state dict)
    cpu = None
    if a.cpu_batch > 0:
        from oracle import nbp_net
        sd = {k: (v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point and "running" not in k))
              for k, v in net.state_dict().items()}
        nb = a.cpu_batch
        xc, gc = xs[:nb].cpu(), gt[:nb].cpu()
        sel = (bidx < nb).cpu()
        cc, gn, bi = coords.cpu()[sel], gains.cpu()[sel], bidx.cpu()[sel]
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        t0 = time.perf_counter()
        o1, o2 = nbp_net.nbp_forward(sd, xc, train=True)
        l = nbp_net.nbp_loss(sd["log_vars"], o1[bi, cc[:, 0], cc[:, 1], cc[:, 2]], gn, o2, gc)
        l.backward()
        cpu_dt = time.perf_counter() - t0
        cpu = {"value": round(nb / cpu_dt, 4), "unit": "maps/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"one fwd+bwd of {nb} maps with torch CPU autograd ({cpu_dt:.1f} s)"}
    print(json.dumps({
        "metric": f"NBP training maps/s (fwd+bwd+AdamW, {a.precision})", "value": round(a.batch / dt, 3), "unit": "maps/s",
        "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 2), "dtype": "f32",
        "train_precision": a.precision, "augment_probability": a.augment, "optimizer": a.optimizer, "grad_clip_norm": a.clip,
        "replay_format": a.replay_format, "ema_decay": a.ema, "ema_updates": None if ema is None else int(ema.num_updates),
        "replay_priority_alpha": a.priority, "replay_priority": None if prio is None else prio.stats(),
        "data": "synthetic", "config": {"workload": f"configs[2]: train step, batch {a.batch} x {a.size}x{a.size}"},
        "tflops_reference_formulation": round(a.batch * flop_map / dt / 1e12, 2), "frac_of_split_ceiling_reference_formulation": round(a.batch * flop_map / dt / (2500e12 / 3), 4),
        "loss": float(loss.item()), "producer_notes": dict(tr.HANDOFF_STATS),
        "cpu_baseline": cpu}))


if __name__ == "__main__":
    main()
