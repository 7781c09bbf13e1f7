#!/usr/bin/env python
"""Validation loss and planner-facing metrics (nextbestpath_amd/utility/metrics.py) of a checkpoint of the NBP trainer.
    python tools/eval_checkpoint.py CHECKPOINT (--store DIR | --synthetic N) [--ema] [--ensemble none|c2|flips|d4]
                                    [--precision fp32_split|fp32] [--thresholds 0.13 ...] [--grid 256] [--batch-size 32] [--num 1200]
CHECKPOINT: a `*_best_val.pth`, a `*_best_val_ema.pth` (its model_state_dict IS the averaged network) or an epoch checkpoint;
--ema takes the averaged weights out of a checkpoint that holds both (`ema_state_dict`).  --store: a replay store of the trainer
(read only: every ceil(total / num)-th record, as the trainer picks its validation set); --synthetic N: N synthetic records of side
--grid.  Runs train_nbp_model.validation_model with the metrics on and prints one JSON object: the loss and the summary.  Two runs
that differ in one flag (--ema, --ensemble, --precision) answer whether that option helps what the planner consumes."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextbestpath_amd.networks.nbp_model import NBP  # noqa: E402
from nextbestpath_amd.trainers import train_nbp_model as T  # noqa: E402


def load_network(path, ema, device):
    ck = torch.load(path, map_location="cpu")
    if ema:
        if "ema_state_dict" not in ck:
            raise SystemExit(f"{path} holds no ema_state_dict (a *_best_val_ema.pth is the averaged network already: drop --ema)")
        sd = ck["ema_state_dict"]["shadow"]
    else:
        sd = ck["model_state_dict"] if "model_state_dict" in ck else ck
    net = NBP()
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval(), ck.get("epoch")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("checkpoint")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--store", help="directory of a replay store")
    src.add_argument("--synthetic", type=int, metavar="N", help="N synthetic validation records")
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--ensemble", choices=["none", "c2", "flips", "d4"], default="none")
    ap.add_argument("--precision", choices=["fp32_split", "fp32"], default=None)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.13])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--num", type=int, default=1200, help="records taken from the store")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "eval_checkpoint runs the network on the GPU only"
    dev = torch.device("cuda", torch.cuda.current_device())
    net, epoch = load_network(a.checkpoint, a.ema, dev)
    if a.precision:
        net.conv_precision = a.precision
    net.symmetry_ensemble = None if a.ensemble == "none" else a.ensemble
    if a.store:
        from nextbestpath_amd.utility import nbp_utils as nu
        env = nu.open_experience_db(a.store)
        records = nu.store_validation_data_readonly(env, num=a.num, keep_compact=True)
        env.close()
    else:
        records = T.make_synthetic_experiences(a.synthetic, a.grid, seed=1)
    if not records:
        raise SystemExit("no validation records")
    acc = T.ValidationMetrics(a.thresholds)
    with torch.no_grad():
        loss = T.validation_model(records, types.SimpleNamespace(nbp_batch_size=a.batch_size), net, dev, metrics=acc)
    out = {"checkpoint": os.path.basename(a.checkpoint), "epoch": epoch, "ema": bool(a.ema), "ensemble": a.ensemble,
           "precision": net.conv_precision, "validation_loss": loss}
    out.update(acc.summary(dev))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
