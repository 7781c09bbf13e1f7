"""NBP training -- host-side mirror of next_best_path/trainers/train_nbp_model.py:40-157 and the
training half of next_best_path/utility/nbp_utils.py (initialize_nbp :213-231, validation_model
:293-338, train_experience_data :340-395, train_nbp :430-468): same function names, same record
schema ('current_model_input', 'current_gt_2d_layout', 'target_value_map_pixel',
'actual_coverage_gain', 'pose_i'), same micro-batch / 8-step gradient accumulation / AdamW /
ReduceLROnPlateau logic.  Forward and backward run on the HIP kernels (networks/training.py).

The replay store and the trajectory collection that fills it live in utility/nbp_utils.py (SURVEY.md 8f
rank 2); ``make_synthetic_experiences`` synthesises records of the same schema for the config-3 benchmark.
Under torchrun every rank collects its own scenes into its own store, trains on its own
samples and the gradients are averaged with bucketed RCCL all-reduces before each optimizer step."""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch

from ..networks import training as tr
from ..networks.nbp_model import NBP
from ..utility import augment, hipops


OPTIMIZERS = ("torch", "hip")


def make_optimizer(nbp, lr=0.001, impl="torch", grad_clip_norm=None, skip_nonfinite_steps=False):
    """The reference's optimizer (nbp_utils.py:228): AdamW(lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight decay 0.01).

    impl "torch" (the default): on the device the update of the 200 MB of parameters runs as torch's FUSED multi-tensor kernel (one
    pass over p, g, m, v instead of the ~10 element-wise passes of the default `foreach` form: 3 % of a B = 32 training step); same
    update rule.  impl "hip": nextbestpath_amd.optim.HipAdamW, the same rule on this project's kernels (csrc/nbp_optim.hip), which
    can also clip the global gradient norm to `grad_clip_norm` (clip_grad_norm_'s coefficient, applied as the gradients are read:
    p.grad itself is left alone) and drop a step whose gradients hold an inf or a NaN (`skip_nonfinite_steps`; what the
    reference's GradScaler does at nbp_utils.py:386-388), both decided on the device without a host synchronisation.  The two
    options exist only there: with impl "torch" they raise instead of being emulated with torch operations."""
    if impl not in OPTIMIZERS:
        raise ValueError(f"optimizer {impl!r}: expected one of {OPTIMIZERS}")
    if grad_clip_norm is not None and not (isinstance(grad_clip_norm, (int, float)) and not isinstance(grad_clip_norm, bool)
                                           and grad_clip_norm > 0 and np.isfinite(grad_clip_norm)):
        raise ValueError(f"grad_clip_norm must be a positive number or None, not {grad_clip_norm!r}")
    kw = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    params = list(nbp.parameters())
    if impl == "hip":
        from ..optim import HipAdamW
        return HipAdamW(params, max_grad_norm=grad_clip_norm, skip_nonfinite=bool(skip_nonfinite_steps), **kw)
    if grad_clip_norm is not None or skip_nonfinite_steps:
        raise ValueError('grad_clip_norm / skip_nonfinite_steps need the HIP optimizer: set "optimizer": "hip" (impl="hip")')
    if params and all(p.is_cuda for p in params):
        try:
            return torch.optim.AdamW(params, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):     # a torch build without the fused kernel
            pass
    return torch.optim.AdamW(params, **kw)


def initialize_nbp(params, nbp, torch_seed=9, initialize=False, pretrained=False, ddp_rank=None):
    """ref nbp_utils.py:213-231: AdamW(lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight decay 0.01).  The config's `optimizer`
    ("torch" | "hip"), `grad_clip_norm` (null | > 0) and `skip_nonfinite_steps` choose make_optimizer's form."""
    opt = make_optimizer(nbp, impl=getattr(params, "optimizer", "torch"), grad_clip_norm=getattr(params, "grad_clip_norm", None),
                         skip_nonfinite_steps=bool(getattr(params, "skip_nonfinite_steps", False)))
    return nbp, opt, 10000.0, 0


def make_ema(params, nbp):
    """The config's `ema_decay` (null = off, the default | a number in [0, 1)) and `ema_warmup` -> None or a
    nextbestpath_amd.optim.WeightEMA of `nbp` (csrc/nbp_ema.hip).  Not in the reference, which keeps no averaged weights: the
    average is an observer of the training run -- validated and checkpointed beside the live weights, which it never changes."""
    decay = getattr(params, "ema_decay", None)
    if decay is None:
        return None
    from ..optim import WeightEMA, check_ema_decay
    return WeightEMA(nbp, check_ema_decay(decay), warmup=bool(getattr(params, "ema_warmup", True)))


def collection_model(params, nbp, ema):
    """The network that acts during trajectory collection: the live one, or with `ema_collect` the averaged one (the role of a
    target network).  The one place where the average changes what the training run computes."""
    if ema is not None and bool(getattr(params, "ema_collect", False)):
        return ema.module
    return nbp


def make_synthetic_experiences(n, S=256, seed=0):
    """Replay records with the reference's schema and the input recipe of SURVEY.md 8d (config 3)."""
    from ..utility.synthetic import make_count_maps
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(1, 41))
        out.append({
            "current_model_input": make_count_maps(1, S, seed=seed * 100003 + i).numpy(),
            "current_gt_2d_layout": (rng.random((1, 1, S, S)) < 0.1).astype(np.float32),
            "target_value_map_pixel": np.stack([rng.integers(0, 8, k), rng.integers(0, S // 4, k),
                                                rng.integers(0, S // 4, k)], 1).astype(np.int64),
            "actual_coverage_gain": rng.uniform(0, 5, k).astype(np.float32),
            "pose_i": int(rng.integers(0, 101)),
        })
    return out


_STAGE_BATCHES = True      # False: every batch through _collate's synchronous copies (the bit-identity tests' reference)


def _expanded(batch_data):
    """Records read with keep_compact=True -> the five-key form (compact ones decoded on the host by the numpy codec)."""
    if any("nbpc" in d for d in batch_data):
        from ..utility.nbp_utils import expand_record
        return [expand_record(d) for d in batch_data]
    return batch_data


def _record_side(d):
    """Side S of a record's maps, in either form."""
    return int(d["S"]) if "nbpc" in d else d["current_model_input"].shape[-1]


def _collate(batch_data, device):
    batch_data = _expanded(batch_data)
    # (np.concatenate, not torch.cat of 32 x 1.3 MB: on a 256-core host torch's intra-op thread pool made that concatenation cost
    # 50-600 ms per batch, tools/diag/train_loop_ab.py)
    xs = torch.from_numpy(np.concatenate([d["current_model_input"] for d in batch_data])).to(device)
    gt = torch.from_numpy(np.concatenate([d["current_gt_2d_layout"] for d in batch_data])).to(device)
    coords = [torch.from_numpy(np.copy(d["target_value_map_pixel"])) for d in batch_data]
    # the reference indexes predicted_value_map[b, c, x, y] (nbp_utils.py:379), which raises on a bad coordinate; the
    # device gather has no exception path, so replay records (possibly written elsewhere) are range-checked here
    V = xs.shape[-1] // 4
    for d, c in zip(batch_data, coords):
        if c.numel() and (c.min() < 0 or c[:, 0].max() >= 8 or c[:, 1:].max() >= V):
            raise IndexError(f"target_value_map_pixel out of range for an [8,{V},{V}] value map (pose_i={d.get('pose_i')})")
    gains = torch.cat([torch.from_numpy(np.copy(d["actual_coverage_gain"])) for d in batch_data]).to(device)
    sizes = torch.tensor([len(c) for c in coords])
    bidx = torch.repeat_interleave(torch.arange(len(coords)), sizes).to(device)
    return xs, gt, torch.cat(coords).to(device), gains, bidx


class _BatchStager:
    """The next batch's host-to-device copies on a stream of their own, from pinned staging buffers (two sets, used alternately), so
    that they run under the current batch's forward / backward instead of in front of the next one's: `.to(device)` from pageable
    memory is host-synchronous AND stream-ordered behind the kernels already queued (the reference pays exactly that,
    nbp_utils.py:352-355).  Same tensors on the device, bit for bit."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device)
        self.pins = [{}, {}]
        self.done = [None, None]
        self.k = 0

    def _pin(self, slot, name, shape, dtype):
        numel = int(np.prod(shape)) if len(shape) else 1
        buf = self.pins[slot].get(name)
        if buf is None or buf.numel() < numel or buf.dtype != dtype:
            buf = self.pins[slot][name] = torch.empty(max(numel, 1), dtype=dtype).pin_memory()
        return buf[:numel].view(shape)

    def begin(self):
        """Next staging slot: waits (host) for the copies that last read its pinned buffers (two batches ago)."""
        self.slot = self.k & 1
        self.k += 1
        if self.done[self.slot] is not None:
            self.done[self.slot].synchronize()
        self.filled = {}

    def buffer(self, name, shape, dtype):
        """A pinned tensor of this slot to be filled by the caller (records are copied straight into it: no torch.cat, whose
        intra-op thread pool made a 42 MB concatenation cost 50 ms on the 256-core host)."""
        t = self._pin(self.slot, name, tuple(shape), dtype)
        self.filled[name] = t
        return t

    def commit(self):
        """-> ({name: device tensor}, event the consumer's stream must wait for)"""
        out = {}
        with torch.cuda.stream(self.stream):
            for name, p in self.filled.items():
                out[name] = torch.empty(p.shape, dtype=p.dtype, device=self.device)
                out[name].copy_(p, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.done[self.slot] = ev
        return out, ev


def _with_extras(out, dev, ops, weights):
    """The staged tensors, then the op codes, then the weights -- each only when the batch has them."""
    if ops is not None:
        out = out + (dev["ops"],)
    if weights is not None:
        out = out + (dev["weights"],)
    return out


def _collate_staged(batch_data, device, stager, ops=None, weights=None):
    """_collate with the copies on the stager's stream: returns the same five tensors; the CURRENT stream waits for them.
    `ops` (augmentation op codes, int32 [n]; None without augmentation) ride along as a sixth tensor, `weights` (the replay draw's
    importance weights, fp32 [n]; None without prioritised replay) behind them."""
    n = len(batch_data)
    x0 = batch_data[0]["current_model_input"]
    S = x0.shape[-1]
    coords = [np.asarray(d["target_value_map_pixel"]) for d in batch_data]
    V = S // 4
    for d, c in zip(batch_data, coords):
        if c.size and (c.min() < 0 or c[:, 0].max() >= 8 or c[:, 1:].max() >= V):
            raise IndexError(f"target_value_map_pixel out of range for an [8,{V},{V}] value map (pose_i={d.get('pose_i')})")
    K = int(sum(len(c) for c in coords))
    stager.begin()
    xs = stager.buffer("xs", (n,) + tuple(x0.shape[1:]), torch.float32).numpy()
    gt = stager.buffer("gt", (n,) + tuple(batch_data[0]["current_gt_2d_layout"].shape[1:]), torch.float32).numpy()
    cd = stager.buffer("coords", (K, 3), torch.int64).numpy()
    gn = stager.buffer("gains", (K,), torch.float32).numpy()
    bi = stager.buffer("bidx", (K,), torch.int64).numpy()
    if ops is not None:
        stager.buffer("ops", (n,), torch.int32).numpy()[:] = ops
    if weights is not None:
        stager.buffer("weights", (n,), torch.float32).numpy()[:] = weights
    k = 0
    for i, (d, c) in enumerate(zip(batch_data, coords)):
        xs[i] = d["current_model_input"][0]
        gt[i] = d["current_gt_2d_layout"][0]
        m = len(c)
        cd[k:k + m] = c
        gn[k:k + m] = d["actual_coverage_gain"]
        bi[k:k + m] = i
        k += m
    dev, ev = stager.commit()
    out = (dev["xs"], dev["gt"], dev["coords"], dev["gains"], dev["bidx"])
    return _with_extras(out, dev, ops, weights), ev


class _PendingDecode:
    """The images of a batch of compact records on their way to the device: the streams back to back in one staged uint8 buffer.
    `finish` expands them with one launch (hipops.replay_decode) on the CURRENT stream, which must have waited for the stager's
    event: the same xs / gt tensors, bit for bit, as the reference-format records' staged copy."""

    def __init__(self, streams, offsets, S):
        self.streams, self.offsets, self.S = streams, offsets, S

    def finish(self, device):
        self.streams.record_stream(torch.cuda.current_stream(device))
        return hipops.replay_decode(self.streams, self.offsets, self.S)


def _collate_compact(batch_data, device, stager, ops=None, weights=None):
    """_collate_staged for a batch whose records are all compact (unpack_record(..., keep_compact=True): headers validated): the
    streams go back to back, each padded to 16 bytes, into one pinned uint8 staging buffer -- a few per cent of the 1.3 MB per record
    of the expanded maps through pinned memory and over the host-to-device link; targets, gains, indices and op codes as ever.
    -> ((_PendingDecode, None, coords, gains, bidx[, ops]), event); _await_batch turns the first two into xs and gt."""
    n = len(batch_data)
    S = _record_side(batch_data[0])
    if any(_record_side(d) != S for d in batch_data):
        raise ValueError("replay records of different map sizes in one batch")
    coords = [np.asarray(d["target_value_map_pixel"]) for d in batch_data]
    V = S // 4
    for d, c in zip(batch_data, coords):
        if c.size and (c.min() < 0 or c[:, 0].max() >= 8 or c[:, 1:].max() >= V):
            raise IndexError(f"target_value_map_pixel out of range for an [8,{V},{V}] value map (pose_i={d.get('pose_i')})")
    K = int(sum(len(c) for c in coords))
    offsets, total = [], 0
    for d in batch_data:
        offsets.append(total)
        total += (len(d["nbpc"]) + 15) & ~15
    stager.begin()
    buf = stager.buffer("streams", (total,), torch.uint8).numpy()
    cd = stager.buffer("coords", (K, 3), torch.int64).numpy()
    gn = stager.buffer("gains", (K,), torch.float32).numpy()
    bi = stager.buffer("bidx", (K,), torch.int64).numpy()
    if ops is not None:
        stager.buffer("ops", (n,), torch.int32).numpy()[:] = ops
    if weights is not None:
        stager.buffer("weights", (n,), torch.float32).numpy()[:] = weights
    k = 0
    for i, (d, c) in enumerate(zip(batch_data, coords)):
        m = len(d["nbpc"])
        buf[offsets[i]:offsets[i] + m] = np.frombuffer(d["nbpc"], dtype=np.uint8)
        buf[offsets[i] + m:offsets[i + 1] if i + 1 < n else total] = 0
        m = len(c)
        cd[k:k + m] = c
        gn[k:k + m] = d["actual_coverage_gain"]
        bi[k:k + m] = i
        k += m
    dev, ev = stager.commit()
    out = (_PendingDecode(dev["streams"], offsets, S), None, dev["coords"], dev["gains"], dev["bidx"])
    return _with_extras(out, dev, ops, weights), ev


def _await_batch(tensors, ev, device):
    """The consumer's side of a staged batch: the current stream waits for the copies, keeps their buffers, and expands a compact
    batch's streams.  -> the tensors, xs and gt first."""
    cur = torch.cuda.current_stream(device)
    cur.wait_event(ev)
    pending = tensors[0] if isinstance(tensors[0], _PendingDecode) else None
    for t in tensors[2 if pending else 0:]:
        t.record_stream(cur)
    if pending:
        tensors = pending.finish(device) + tuple(tensors[2:])
    return tensors


def _collate_any(batch_data, device, stager, ops=None, weights=None):
    """Staged collation for records of the replay store's shape (one map per record); anything else through _collate.  A batch of
    compact records only goes to the device as streams (_collate_compact); a batch that mixes the formats has its compact records
    decoded on the host first."""
    extra = {} if weights is None else {"weights": weights}
    if all("nbpc" in d for d in batch_data):
        return _collate_compact(batch_data, device, stager, ops, **extra)
    batch_data = _expanded(batch_data)
    if all(d["current_model_input"].shape[0] == 1 and d["current_gt_2d_layout"].shape[0] == 1 for d in batch_data):
        return _collate_staged(batch_data, device, stager, ops, **extra)
    ev = torch.cuda.Event()
    out = _collate(batch_data, device)
    if ops is not None:
        out = out + (torch.from_numpy(np.asarray(ops, dtype=np.int32)).to(device),)
    if weights is not None:
        out = out + (torch.from_numpy(np.asarray(weights, dtype=np.float32)).to(device),)
    ev.record(torch.cuda.current_stream(device))
    return out, ev


BUCKET_BYTES = 64 << 20      # xGMI rings are per-link bound (~153 GB/s): 4 buckets cover the 200 MB of gradients


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None      # also a 1-rank group (RCCL on one GPU)


def allreduce_gradients(nbp):
    """Averages the accumulated gradients over the ranks: parameters are packed into flat buckets of at most
    BUCKET_BYTES in registration order, one all-reduce (RCCL on ROCm) per bucket."""
    dist = _dist()
    if dist is None:
        return
    world = dist.get_world_size()
    params = [p for p in nbp.parameters() if p.grad is not None]
    i = 0
    while i < len(params):
        bucket, size = [], 0
        while i < len(params) and (not bucket or size + params[i].grad.numel() * 4 <= BUCKET_BYTES):
            bucket.append(params[i]); size += params[i].grad.numel() * 4; i += 1
        flat = torch.cat([p.grad.reshape(-1) for p in bucket])
        if dist.get_backend() == "gloo" and flat.is_cuda:      # CPU rendezvous in tests; RCCL reduces in place on the GPU
            host = flat.cpu()
            dist.all_reduce(host)
            flat.copy_(host)
        else:
            dist.all_reduce(flat)
        flat /= world
        off = 0
        for p in bucket:
            n = p.grad.numel()
            p.grad.copy_(flat[off:off + n].view_as(p.grad)); off += n


def _common_count(n, device):
    """Every rank must take the same number of optimizer steps: min over ranks of the local batch count."""
    dist = _dist()
    if dist is None:
        return n
    t = torch.tensor([n], dtype=torch.int64, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return int(t.item())


def _mean_over_ranks(x: float, device) -> float:
    """Scalars that steer the optimiser (validation loss -> ReduceLROnPlateau) must agree on every rank."""
    dist = _dist()
    if dist is None:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t)
    return float(t.item()) / dist.get_world_size()


def _augment_rng(params):
    """The trainer's own generator for the augmentation draws: one per params object, so that it runs on across the inner epochs
    and never touches the global `random` (which shuffles the replay set).  Seed: `augment_seed`, else random_seed + rank."""
    rng = getattr(params, "_augment_rng", None)
    if rng is None:
        seed = getattr(params, "augment_seed", None)
        if seed is None:
            dist = _dist()
            seed = int(getattr(params, "random_seed", 0)) + (dist.get_rank() if dist is not None else 0)
        rng = random.Random(f"nbp-augment-{int(seed)}")
        params._augment_rng = rng
    return rng


def replay_priority_options(params):
    """The config's `replay_priority_alpha` (null = off, the default | a number >= 0; 0.6 is the paper's), `replay_priority_beta`
    (0.4, in [0, 1]), `replay_priority_eps` (1e-3, > 0) and `replay_priority_seed` (null = random_seed + rank) -> None, or the
    checked values (utility/priority.py::check_options; ValueError on a bad one)."""
    from ..utility import priority
    return priority.check_options(getattr(params, "replay_priority_alpha", None), getattr(params, "replay_priority_beta", 0.4),
                                  getattr(params, "replay_priority_eps", 1e-3), getattr(params, "replay_priority_seed", None))


def make_replay_priorities(params):
    """None with the option off, else a fresh utility/priority.py::ReplayPriorities (run_training_nbp keeps one per rank for the run)."""
    opts = replay_priority_options(params)
    if opts is None:
        return None
    from ..utility.priority import ReplayPriorities
    return ReplayPriorities(opts["alpha"], opts["beta"], opts["eps"])


def _priority_rng(params, opts):
    """The generator of the replay draws: one per params object, as the augmentation's; seed `replay_priority_seed`, else
    random_seed + rank."""
    rng = getattr(params, "_priority_rng", None)
    if rng is None:
        seed = opts["seed"]
        if seed is None:
            dist = _dist()
            seed = int(getattr(params, "random_seed", 0)) + (dist.get_rank() if dist is not None else 0)
        rng = params._priority_rng = np.random.default_rng(int(seed))
    return rng


def train_experience_data(training_set_db, params, optimizer, nbp, device, current_epoch, grad_norms=None, ema=None, priorities=None):
    """ref nbp_utils.py:340-395 (GradScaler without autocast is the identity scale for fp32; omitted -- the "fp16"
    train_precision scales every fp16 operand per tensor instead, NBP.train_precision).  As in the
    reference the early poses (pose_i <= 10) are dropped INSIDE each batch during epoch 1 (:348-362), a batch left empty
    is skipped before the optimiser-step test (:364-365), and the step fires every 8 non-empty batches or on the batch
    that reaches the end of the set (:385).  Under torchrun the ranks agree on "empty" and on the batch count, because
    the step contains the gradient all-reduce.

    Not in the reference's loop (its augment_data, nbp_utils.py:267-289, is never called): with params.augment_probability = p > 0
    every sample is moved, with probability p, by one of the seven non-identity symmetries of the square about the camera
    (utility/augment.py) -- the targets' cells and heading channels on the host before collation, on shallow copies of the records,
    the six planes on the device behind the staged copy (one launch, hipops.augment_batch).  p = 0 (the default) draws nothing and
    launches nothing.  `ema` (make_ema; None = off) is updated once per optimizer step, right behind it on the stream; with the HIP
    optimizer a step dropped on the device drops the update too.

    Not in the reference either: loss-prioritised replay (utility/priority.py; Schaul et al. 2016), with params.replay_priority_alpha
    set (null, the default: everything above, bit for bit -- nothing new launched, drawn or written).  The population is the list
    itself (in epoch 1 without the records of pose_i <= 10, the ones the in-batch filter drops); instead of a shuffle,
    ceil(N / batch size) batches are DRAWN with replacement from `priorities` (a ReplayPriorities: the caller's, kept over the run,
    else one kept on `params`), the last one with the remainder, so that an inner epoch still trains on N samples.  A record's key
    is its store key d["_key"] (read_combined_data(with_keys=True)) or, without one, its position in the list.  The draw's weights
    travel with the staged batch, the objective is tr.loss_weighted, and every batch's per-sample terms stay on the device until
    the optimizer step's read-back, which grows by ONE device-to-host copy per optimizer step (the window's per-sample terms and
    log_vars as they were before the step); the table is then updated with priority.sample_loss.  The batch prefetched under the
    current one is drawn from the table as it stands: the priorities LAG by up to one accumulation window (8 batches) plus the
    prefetched batch.  Augmentation composes unchanged (the draw picks records, the augmentation then moves them).  Under torchrun
    each rank draws from its own records; the batch count goes through _common_count as ever."""
    prio = replay_priority_options(params)
    if prio is not None:
        return _train_prioritised(training_set_db, params, optimizer, nbp, device, current_epoch, grad_norms, ema, priorities, prio)
    random.shuffle(training_set_db)
    aug_p = float(getattr(params, "augment_probability", 0.0) or 0.0)
    if not 0.0 <= aug_p <= 1.0:
        raise ValueError(f"augment_probability {aug_p} outside [0, 1]")
    aug_rng = _augment_rng(params) if aug_p > 0 else None
    # the batch losses of an accumulation window stay on the device until its optimizer step (the reference's `batch_loss.item()`
    # per batch, nbp_utils.py:384, is a device synchronisation per batch: the GPU then idles through the next batch's collation and
    # host-to-device copy).  Same numbers: the same fp32 losses, converted and added as Python floats in the same order.
    training_loss, pending, updates = [], [], 0
    accumulation_steps = 8
    bs = params.nbp_batch_size
    n_batches = _common_count((len(training_set_db) + bs - 1) // bs, device)
    multi_rank = _dist() is not None
    stager = _BatchStager(device) if (torch.device(device).type == "cuda" and _STAGE_BATCHES) else None

    def batch_of(bi):
        batch = training_set_db[bi * bs:(bi + 1) * bs]
        if current_epoch == 1:
            batch = [d for d in batch if d["pose_i"] > 10]
        return batch

    def augmented(batch):
        """-> (records with their targets moved, op codes) -- (batch, None) without augmentation"""
        if aug_rng is None:
            return batch, None
        ops = augment.draw_ops(aug_rng, len(batch), aug_p)
        return augment.augment_records(batch, ops, _record_side(batch[0]) // 4), ops

    staged = None            # (batch index, tensors, event) of the batch whose copies were started under the previous one's compute
    for bi in range(n_batches):
        batch = batch_of(bi)
        have = 1 if batch else 0
        if multi_rank:
            have = _common_count(have, device)
        if not have:
            continue
        if stager is None:
            batch, ops = augmented(batch)
            xs, gt, coords, gains, bidx = _collate(batch, device)
            if ops is not None:
                ops = torch.from_numpy(ops).to(device)
        else:
            if staged is None or staged[0] != bi:
                batch, ops = augmented(batch)
                staged = (bi,) + _collate_any(batch, device, stager, ops)
            tensors = _await_batch(staged[1], staged[2], device)
            xs, gt, coords, gains, bidx = tensors[:5]
            ops = tensors[5] if len(tensors) > 5 else None
        if ops is not None:
            xs, gt = hipops.augment_batch(xs, gt, ops)
        out1, out2 = nbp(xs)
        pred = tr.gather_values(out1, bidx, coords)
        loss = nbp.loss(pred, gains, out2, gt)
        loss.backward()
        pending.append(loss.detach())
        updates += 1
        if stager is not None and bi + 1 < n_batches:       # the next batch's collation and copies, under this batch's kernels
            nb = batch_of(bi + 1)
            if nb:
                nb, nops = augmented(nb)
                staged = (bi + 1,) + _collate_any(nb, device, stager, nops)
            else:
                staged = None
        if updates % accumulation_steps == 0 or bi + 1 == n_batches:
            allreduce_gradients(nbp)
            optimizer.step()
            if ema is not None:
                ema.update(optimizer)
            optimizer.zero_grad()
            accumulated = 0.0
            with_norm = bool(getattr(optimizer, "norm_pass", False))
            values = torch.stack(pending + [optimizer.last_grad_norm] if with_norm else pending).tolist()   # (one device -> host copy per optimizer step)
            if with_norm:
                norm = values.pop()
                if grad_norms is not None:
                    grad_norms.append(norm)
            for v in values:
                accumulated += v
            training_loss.append(accumulated / accumulation_steps)
            pending, updates = [], 0
    return training_loss


def _train_prioritised(training_set_db, params, optimizer, nbp, device, current_epoch, grad_norms, ema, priorities, prio):
    """train_experience_data with replay_priority_alpha set (its docstring): same accumulation, optimizer step and loss list."""
    from ..utility import priority
    aug_p = float(getattr(params, "augment_probability", 0.0) or 0.0)
    if not 0.0 <= aug_p <= 1.0:
        raise ValueError(f"augment_probability {aug_p} outside [0, 1]")
    aug_rng = _augment_rng(params) if aug_p > 0 else None
    if priorities is None:
        priorities = getattr(params, "_replay_priorities", None)
        if priorities is None:
            priorities = params._replay_priorities = make_replay_priorities(params)
    rng = _priority_rng(params, prio)
    keep = [i for i, d in enumerate(training_set_db) if current_epoch != 1 or d["pose_i"] > 10]
    population = [training_set_db[i] for i in keep]
    priorities.begin([training_set_db[i].get("_key", i) for i in keep])
    N = len(population)
    training_loss, pending, window, updates = [], [], [], 0
    accumulation_steps = 8
    bs = params.nbp_batch_size
    n_batches = _common_count((N + bs - 1) // bs, device)
    stager = _BatchStager(device) if (torch.device(device).type == "cuda" and _STAGE_BATCHES) else None

    def drawn(bi):
        """-> (records, their keys, weights fp32, op codes or None) of batch bi, drawn from the table as it stands"""
        idx, w = priorities.draw(rng, min(bs, N - bi * bs))
        batch = [population[i] for i in idx]
        keys = [priorities.keys[i] for i in idx]
        ops = None
        if aug_rng is not None:
            ops = augment.draw_ops(aug_rng, len(batch), aug_p)
            batch = augment.augment_records(batch, ops, _record_side(batch[0]) // 4)
        return batch, keys, w.astype(np.float32), ops

    staged = None            # (batch index, keys, tensors, event) of the batch whose copies were started under the previous one's compute
    for bi in range(n_batches):
        if stager is None:
            batch, keys, w, ops = drawn(bi)
            xs, gt, coords, gains, bidx = _collate(batch, device)
            ops = None if ops is None else torch.from_numpy(ops).to(device)
            w = torch.from_numpy(w).to(device)
        else:
            if staged is None or staged[0] != bi:
                batch, keys, w, ops = drawn(bi)
                staged = (bi, keys) + _collate_any(batch, device, stager, ops, weights=w)
            keys = staged[1]
            tensors = _await_batch(staged[2], staged[3], device)
            xs, gt, coords, gains, bidx = tensors[:5]
            extras = list(tensors[5:])
            ops = extras.pop(0) if aug_rng is not None else None
            w = extras.pop(0)
        if ops is not None:
            xs, gt = hipops.augment_batch(xs, gt, ops)
        out1, out2 = nbp(xs)
        loss, per_sample = tr.loss_weighted(nbp, out1, bidx, coords, gains, out2, gt, w)
        loss.backward()
        pending.append(loss.detach())
        window.append((keys, per_sample, xs.shape[-1]))
        updates += 1
        if stager is not None and bi + 1 < n_batches:       # the next batch's draw, collation and copies, under this batch's kernels
            nb, nkeys, nw, nops = drawn(bi + 1)
            staged = (bi + 1, nkeys) + _collate_any(nb, device, stager, nops, weights=nw)
        if updates % accumulation_steps == 0 or bi + 1 == n_batches:
            # the window's per-sample terms and the log_vars they were formed with, gathered on the device BEFORE the step changes them
            terms = torch.cat([ps.reshape(-1) for _, ps, _ in window] + [nbp.log_vars.detach().to(torch.float64)])
            allreduce_gradients(nbp)
            optimizer.step()
            if ema is not None:
                ema.update(optimizer)
            optimizer.zero_grad()
            accumulated = 0.0
            with_norm = bool(getattr(optimizer, "norm_pass", False))
            values = torch.stack(pending + [optimizer.last_grad_norm] if with_norm else pending).tolist()   # (the read-back as ever)
            terms = terms.cpu().numpy()                                                                    # (and the ONE more copy)
            if with_norm:
                norm = values.pop()
                if grad_norms is not None:
                    grad_norms.append(norm)
            for v in values:
                accumulated += v
            training_loss.append(accumulated / accumulation_steps)
            log_vars, at = terms[-2:], 0
            for keys, ps, S in window:
                n = ps.shape[0]
                priorities.update(keys, priority.sample_loss(terms[at:at + 3 * n].reshape(n, 3), S, log_vars))
                at += 3 * n
            pending, window, updates = [], [], 0
    return training_loss


def sync_buffers(nbp):
    """BatchNorm running statistics are per rank during training; before validation / checkpointing they are averaged so
    that every rank evaluates (and rank 0 saves) the same eval-mode network.  No-op without torch.distributed."""
    dist = _dist()
    if dist is None:
        return
    world = dist.get_world_size()
    for name, buf in nbp.named_buffers():
        if buf.dtype.is_floating_point:
            t = buf.data if dist.get_backend() == "nccl" else buf.data.cpu()
            dist.all_reduce(t)
            buf.data.copy_(t / world)
        # num_batches_tracked: identical on every rank (same number of forward passes)


def metric_thresholds(params):
    """The config's `validation_metrics` (false = off, the default) and `metric_thresholds` ([0.13]) -> None, or the checked tuple of
    thresholds of the obstacle mask."""
    if not bool(getattr(params, "validation_metrics", False)):
        return None
    from ..utility import metrics
    return metrics.check_thresholds(getattr(params, "metric_thresholds", metrics.DEFAULT_THRESHOLDS))


class ValidationMetrics:
    """Accumulator of the planner-facing validation metrics (utility/metrics.py) for validation_model: `add` computes a batch's three
    per-sample arrays on the device (hipops.validation_metrics: no synchronisation) and keeps them there; `read` brings all of
    them to the host in ONE copy and adds their raw sums to `totals`; `summary` sums the totals over the ranks of a
    torch.distributed job (one all_reduce of a float64 vector: counts far below 2^53, exact) and forms the ratios."""

    def __init__(self, thresholds=(0.13,)):
        from ..utility import metrics
        self.thresholds = metrics.check_thresholds(thresholds)
        self.totals = np.zeros(metrics.totals_size(len(self.thresholds)), np.float64)
        self._pending = []

    def add(self, out1, out2, gt, coords, gains, bidx):
        self._pending.append(hipops.validation_metrics(out1.detach(), out2.detach(), gt, coords, gains, bidx, self.thresholds))

    def read(self):
        from ..utility import metrics
        if not self._pending:
            return
        T, sizes = len(self.thresholds), [o.shape[0] for o, _, _ in self._pending]
        # (the float64 sums travel as their bit patterns beside the integers: one device -> host copy for the whole loop)
        flat = torch.cat([t.reshape(-1) if t.dtype == torch.int64 else t.reshape(-1).view(torch.int64)
                          for group in zip(*self._pending) for t in group]).cpu().numpy()
        self._pending = []
        n = sum(sizes)
        obst = flat[:n * T * 4].reshape(n, T, 4)
        rank = flat[n * T * 4:n * (T * 4 + 6)].reshape(n, 6)
        val = flat[n * (T * 4 + 6):].view(np.float64).reshape(n, 4)
        self.totals += metrics.totals(obst, rank, val)

    def summary(self, device=None):
        from ..utility import metrics
        self.read()
        tot = self.totals
        dist = _dist()
        if dist is not None:
            t = torch.from_numpy(tot.copy())
            if dist.get_backend() == "nccl":
                t = t.to(device)
            dist.all_reduce(t)
            tot = t.cpu().numpy()
        return metrics.summarize_totals(tot, self.thresholds)


def validation_model(training_set_db, params, nbp, device, metrics=None):
    """ref nbp_utils.py:293-338: plain MSE + BCE in eval mode.  metrics: None, or a ValidationMetrics that receives every batch
    (two more launches per batch, kept on the device; read back once behind the loop); the returned loss is the same float."""
    parts, count = [], 0
    bs = params.nbp_batch_size
    stager = _BatchStager(device) if (torch.device(device).type == "cuda" and _STAGE_BATCHES) else None
    for i in range(0, len(training_set_db), bs):
        if stager is None:
            xs, gt, coords, gains, bidx = _collate(training_set_db[i:i + bs], device)
        else:
            tensors, ev = _collate_any(training_set_db[i:i + bs], device, stager)
            xs, gt, coords, gains, bidx = _await_batch(tensors, ev, device)
        out1, out2 = nbp(xs)
        pred = tr.gather_values(out1, bidx, coords)
        parts.append((tr.MeanLossFn.apply(pred, gains, 0) + tr.MeanLossFn.apply(out2, gt, 1)).detach())    # (no sync per batch)
        if metrics is not None:
            metrics.add(out1, out2, gt, coords, gains, bidx)
        count += 1
    if metrics is not None:
        metrics.read()
    total = 0.0
    for v in (torch.stack(parts).tolist() if parts else []):
        total += v
    return total / max(count, 1)


def _with(acc):
    """validation_model's extra keyword: none at all with the metrics off (the call as it always was)."""
    return {} if acc is None else {"metrics": acc}


def train_nbp(training_set_db, params, optimizer, nbp, device, current_epoch, validation_data, lr_patience=2,
              lr_factor=0.1, num_epochs=5, grad_norms=None, ema=None, ema_losses=None, metrics_out=None, priorities=None):
    """ref nbp_utils.py:430-468: 5 inner epochs, validation after each, ReduceLROnPlateau.  grad_norms: see train_experience_data.
    With `ema` the averaged network is validated after each inner epoch as well (same data, same function) and `ema_losses`, a
    list, receives its loss; the scheduler and the returned pair see the live network only.  With the config's `validation_metrics`
    on and `metrics_out`, a dict, the validation of the LAST inner epoch -- the network that gets checkpointed -- also computes the
    planner-facing metrics (ValidationMetrics): metrics_out["validation_metrics"], and with `ema` ["validation_metrics_ema"].
    `priorities`: the run's ReplayPriorities with `replay_priority_alpha` set (train_experience_data), None otherwise."""
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=lr_factor, patience=lr_patience)
    tl, vl = [], []
    thresholds = metric_thresholds(params) if metrics_out is not None else None
    for inner in range(num_epochs):
        acc = ValidationMetrics(thresholds) if (thresholds is not None and inner + 1 == num_epochs) else None
        nbp.train()
        losses = train_experience_data(training_set_db, params, optimizer, nbp, device, current_epoch, grad_norms, ema=ema,
                                       **({} if priorities is None else {"priorities": priorities}))
        tl.append(float(np.mean(losses)) if losses else float("nan"))
        sync_buffers(nbp)
        nbp.eval()
        with torch.no_grad():
            vl.append(_mean_over_ranks(validation_model(validation_data, params, nbp, device, **_with(acc)), device))
        if acc is not None:
            metrics_out["validation_metrics"] = acc.summary(device)
        if ema is not None:
            shadow = ema.module
            sync_buffers(shadow)
            acc = ValidationMetrics(thresholds) if acc is not None else None
            with torch.no_grad():
                ve = _mean_over_ranks(validation_model(validation_data, params, shadow, device, **_with(acc)), device)
            if ema_losses is not None:
                ema_losses.append(ve)
            if acc is not None:
                metrics_out["validation_metrics_ema"] = acc.summary(device)
        sched.step(vl[-1])
    return sum(tl) / len(tl), sum(vl) / len(vl)


def run_training_nbp(params):
    """ref train_nbp_model.py:40-157.  With a dataset at params.data_path: epoch 0 collects trajectories and
    moves the validation records out of the store, every later epoch collects again and trains on
    read_combined_data; without one (offline benchmark mode) the records are synthesised."""
    from ..parallel_rollout import init_distributed
    from ..simulator import scene as sim_scene
    from ..utility import nbp_utils as nu
    prio_opts = replay_priority_options(params)                   # (a bad value raises before any work)
    rank, world, local_rank = init_distributed()
    device = torch.device("cuda", local_rank if world > 1 else getattr(params, "numGPU", 0))
    torch.cuda.set_device(device)
    random.seed(params.random_seed + rank); np.random.seed(params.random_seed + rank); torch.manual_seed(params.torch_seed)
    nbp = NBP().to(device)
    # the training step's arithmetic (NBP.train_precision): "fp32_split" or "fp16" (scaled fp16 mixed precision); the
    # checkpoints are fp32 state_dicts either way
    nbp.train_precision = getattr(params, "train_precision", "fp32_split")
    nbp, optimizer, best_loss, _ = initialize_nbp(params, nbp, params.torch_seed)
    ema = make_ema(params, nbp)          # None unless `ema_decay` is set
    best_ema_loss = best_loss
    S = getattr(params, "grid_size", 256)
    os.makedirs(params.output_dir, exist_ok=True)
    data_path = getattr(params, "data_path", None)
    collect = bool(getattr(params, "collect", True)) and data_path and os.path.isdir(data_path)
    history = {}

    with_norm = bool(getattr(optimizer, "norm_pass", False))      # the HIP optimizer with clipping or skipping on

    with_metrics = metric_thresholds(params) is not None          # `validation_metrics`: off = nothing new launched or written
    # `replay_priority_alpha`: one table per rank for the whole run, so that a record drawn again in a later outer epoch keeps its
    # priority (kept in memory only: not checkpointed); off = None, and nothing new drawn, launched or written
    priorities = make_replay_priorities(params)

    def train_kw(norms, ema_losses, found):
        kw = dict(num_epochs=params.inner_epochs, grad_norms=norms, ema=ema, ema_losses=ema_losses)
        if with_metrics:
            kw["metrics_out"] = found
        if priorities is not None:
            kw["priorities"] = priorities
        return kw

    def note_priorities(found):
        if priorities is not None:      # the table as the epoch's last inner epoch left it
            found["replay_priority"] = {"alpha": prio_opts["alpha"], "beta": prio_opts["beta"], **priorities.stats()}

    def save(epoch, vl, tl, grad_norms, ema_losses, found):
        nonlocal best_loss, best_ema_loss
        if rank != 0:
            return
        history[epoch] = {"training_loss": tl, "validation_loss": vl}
        if ema is not None:
            history[epoch]["validation_loss_ema"] = sum(ema_losses) / len(ema_losses)
        history[epoch].update(found)         # validation_metrics (and validation_metrics_ema) of the epoch's last inner epoch
        if with_norm:       # one norm per optimizer step of the epoch; the running count of dropped steps (validation has synchronised)
            history[epoch].update(grad_norm=list(grad_norms), skipped_steps=int(optimizer.skipped_steps.item()))
        ck = {"epoch": epoch, "model_state_dict": nbp.state_dict(), "optimizer_state_dict": optimizer.state_dict()}
        if "validation_metrics" in found:
            ck["validation_metrics"] = found["validation_metrics"]
        if ema is not None:
            ck["ema_state_dict"] = ema.state_dict()
            vle = history[epoch]["validation_loss_ema"]
            if vle < best_ema_loss:      # the averaged weights as a checkpoint of their own: model_state_dict IS the shadow's
                best_ema_loss = vle
                best = {"epoch": epoch, "model_state_dict": ck["ema_state_dict"]["shadow"], "validation_loss_ema": vle}
                if "validation_metrics_ema" in found:
                    best["validation_metrics"] = found["validation_metrics_ema"]
                torch.save(best, os.path.join(params.output_dir, params.nbp_model_name + "_best_val_ema.pth"))
        if vl < best_loss:
            best_loss = vl
            torch.save(ck, os.path.join(params.output_dir, params.nbp_model_name + "_best_val.pth"))
        if epoch % 3 == 0:
            torch.save(ck, os.path.join(params.output_dir, f"{params.nbp_model_name}_epoch{epoch}.pth"))
        with open(os.path.join(params.output_dir, "loss.json"), "w") as fh:
            json.dump(history, fh)

    if not collect:
        validation = make_synthetic_experiences(getattr(params, "n_validation_synthetic", 16), S, seed=1)
        for epoch in range(1, params.epochs + 1):
            db = make_synthetic_experiences(params.samples_per_epoch, S, seed=100 + epoch + 1000 * rank)
            norms, ema_losses, found = [], [], {}
            tl, vl = train_nbp(db, params, optimizer, nbp, device, epoch, validation, **train_kw(norms, ema_losses, found))
            note_priorities(found)
            print(f"epoch {epoch}: training {tl:.4f} validation {vl:.4f}")
            save(epoch, vl, tl, norms, ema_losses, found)
        return history

    dataset = sim_scene.SceneDataset(data_path, getattr(params, "train_scenes", []))
    db_dir = getattr(params, "db_path", os.path.join(params.output_dir, "db"))
    env = nu.open_experience_db(os.path.join(db_dir, f"{params.nbp_model_name}.rank{rank}"))
    validation = None
    for epoch in range(0, params.epochs + 1):
        cov = []
        with torch.no_grad():
            n = nu.trajectory_collection(params, epoch, dataset, env, (S, S), (S // 4, S // 4), (-40 * S // 256, 40 * S // 256),
                                         collection_model(params, nbp, ema), cov, None, device, rank=rank, world=world,
                                         n_poses=getattr(params, "n_collect_poses", 100),
                                         n_gt_points=getattr(params, "n_gt_surface_points", 50000),
                                         rollouts_per_gpu=getattr(params, "collect_rollouts_per_gpu", 1),
                                         depth_noise=getattr(params, "collect_depth_noise", None),
                                         depth_filter=getattr(params, "collect_depth_filter", None))
        print(f"[rank {rank}] epoch {epoch}: collected {n} records ({env.entries()} in the store)")
        if epoch == 0:
            validation = nu.store_validation_data(env, getattr(params, "n_validation", 1200), keep_compact=True)
            continue
        # (compact records stay streams in host memory and are expanded on the device, batch by batch: _collate_compact)
        keyed = {} if priorities is None else {"with_keys": True}
        db = (nu.read_combined_data(env, sample_m=None, keep_compact=True, **keyed) if epoch == 1
              else nu.read_combined_data(env, keep_compact=True, **keyed))   # ref :436-440
        # every rank must take the same branch (the training loop below contains collectives)
        if _common_count(1 if (db and validation) else 0, device) == 0:
            continue
        norms, ema_losses, found = [], [], {}
        tl, vl = train_nbp(db, params, optimizer, nbp, device, epoch, validation, **train_kw(norms, ema_losses, found))
        note_priorities(found)
        print(f"epoch {epoch}: training {tl:.4f} validation {vl:.4f}")
        save(epoch, vl, tl, norms, ema_losses, found)
    env.close()
    return history
