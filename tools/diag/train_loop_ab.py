"""Diagnostic (GPU box): train_experience_data (the trainer's epoch loop: collation, host-to-device copies, forward, backward, an AdamW step every
8 batches) on host-resident replay records, batch 32 x 256 x 256 -- maps/s with the batches staged on a copy stream and the losses kept on the device
until the optimizer step (_STAGE_BATCHES = True, default) against the reference's loop shape (False: synchronous copies; and, for the record, its
per-batch loss.item(), which round 6 removed in both modes)."""
import os, sys, time, types, random
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from nextbestpath_amd.networks.nbp_model import NBP
from nextbestpath_amd.trainers import train_nbp_model as T

D = torch.device("cuda")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
params = types.SimpleNamespace(nbp_batch_size=32)
db = T.make_synthetic_experiences(n, S=256, seed=5)
torch.manual_seed(3); random.seed(3); np.random.seed(3)
net = NBP().to(D).train()
_, opt, _, _ = T.initialize_nbp(params, net)
for mode in (1, 0, 1, 0):
    T._STAGE_BATCHES = bool(mode)
    T.train_experience_data(list(db[:64]), params, opt, net, D, current_epoch=2)      # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.train_experience_data(list(db), params, opt, net, D, current_epoch=2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"staged batches = {mode}: {n / dt:.1f} maps/s over an epoch of {n} records ({1e3 * dt / (n / 32):.1f} ms per batch of 32)", flush=True)
