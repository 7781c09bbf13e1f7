"""AdamW on the HIP kernels of csrc/nbp_optim.hip, with global-norm gradient clipping and non-finite step skipping on the device.

Reference: next_best_path/utility/nbp_utils.py:228 (``torch.optim.AdamW(lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight decay 0.01)``)
and :386-388 (``scaler.step(optimizer); scaler.update()``: a GradScaler drops a step whose gradients hold an inf or a NaN).

``HipAdamW`` takes ``torch.optim.AdamW``'s arguments plus

  max_grad_norm    None (off) or a positive number: the gradients enter the update multiplied by
                   ``min(1, max_grad_norm / (total_norm + 1e-6))`` -- ``torch.nn.utils.clip_grad_norm_``'s coefficient.  Unlike
                   ``clip_grad_norm_`` the tensors in ``p.grad`` are NOT modified: the coefficient is applied as they are read.
  skip_nonfinite   True: a step whose gradients hold an inf or a NaN writes nothing (``p``, ``exp_avg``, ``exp_avg_sq`` and ``step``
                   stay bit for bit) and ``skipped_steps`` counts it.

A ``step()`` is two or three launches on the current stream (the gradient-norm pass only when one of the two options is on, the
one-workgroup finalize, one update launch per param group) and never waits for the device: the norm, the coefficient, the step
counter and the bias corrections live in a small device block the update kernel reads.  ``last_grad_norm`` and ``skipped_steps`` are
0-dim device tensors (views of that block); read them when something else is read back anyway.

The kernels take their work from two device tables (one record per tensor, one per 16384-element chunk) that are built at the
first step and rebuilt only when an address changes: ``zero_grad(set_to_none=True)`` frees the gradients, so their addresses are
compared at every step (one ``data_ptr()`` per tensor) and, when one moved, the record table is refreshed with one small copy from
pinned memory on the stream.  Dtypes and layouts are validated when the tables are (re)built.

``state[p]`` holds what ``torch.optim.AdamW(fused=True)`` holds -- ``step`` (0-dim fp32 on the device), ``exp_avg``, ``exp_avg_sq`` --
and the param groups carry torch's keys, so a ``state_dict()`` loads into a ``torch.optim.AdamW`` and back.  One step counter serves
every parameter: all parameters that are ever updated must have a gradient from the first step on, and a loaded state whose ``step``
values differ is refused.  There is no CPU path: parameters off the GPU raise ``RuntimeError``.

``WeightEMA`` (below, csrc/nbp_ema.hip) keeps an exponential moving average of a module's weights on the device, gated by the
optimizer's own decision to apply or drop a step.
"""
from __future__ import annotations

import copy
import ctypes

import numpy as np
import torch

from . import _lib

_DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8")])
_CHUNK = np.dtype([("first", "<i8"), ("tensor", "<i4"), ("pad", "<i4")])
# the state block as 32-bit words (include/nbp_hip.h): floats 0 total_norm, 1 clip_coef, 4 step; ints 2 finite, 3 applied, 5 skipped_steps
_W_NORM, _W_STEP, _W_SKIPPED, _W_HEADER = 0, 4, 5, 8
_EMA_DESC = np.dtype([("p", "<u8"), ("e", "<u8"), ("numel", "<i8")])


def _upload(arr, dst=None, device=None):
    """A numpy array to the device through pinned memory, asynchronously on the current stream (torch's host allocator keeps the
    pinned block alive until the copy has run)."""
    src = torch.from_numpy(arr.view(np.uint8).reshape(-1)).pin_memory()
    if dst is None:
        dst = torch.empty(src.numel(), dtype=torch.uint8, device=device)
    dst.copy_(src, non_blocking=True)
    return dst


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None, skip_nonfinite=False):
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("HipAdamW takes lr and betas as Python numbers (they are kernel arguments, read at every step())")
        if amsgrad or maximize or differentiable:
            raise ValueError("HipAdamW has no amsgrad, maximize or differentiable form")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0 and np.isfinite(float(max_grad_norm))):
            raise ValueError(f"max_grad_norm must be a positive finite number or None, not {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._device = None
        self._tables = None          # what the kernels read: see _build
        self._block = None           # the device state block, fp32 words
        self._started = False        # a step has run or a state was loaded: the shared step counter is live
        # torch's own keys (foreach / capturable / fused choose among torch's implementations; here there is one), so that a
        # state_dict moves between this class and torch.optim.AdamW(fused=True) in both directions
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=True, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # ---- construction-time checks (no device work: a CPU parameter must raise on a machine without a GPU too)
    def add_param_group(self, param_group):
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        param_group = dict(param_group, params=ps)
        for p in ps:
            if isinstance(p, tuple) and len(p) == 2:         # (name, parameter), as torch.optim accepts
                p = p[1]
            if not isinstance(p, torch.Tensor):
                raise TypeError("optimizer can only optimize Tensors")
            if not p.is_cuda:
                raise RuntimeError("HipAdamW runs on the GPU only (no CPU fallback): a parameter lives on " + str(p.device))
            if p.is_sparse or p.layout is not torch.strided:
                raise ValueError("HipAdamW does not support sparse parameters")
            if p.dtype != torch.float32:
                raise ValueError(f"HipAdamW updates fp32 parameters only (the kernels are fp32), not {p.dtype}")
            if not p.is_contiguous():
                raise ValueError("HipAdamW needs contiguous parameters")
            if self._device is None:
                self._device = p.device
            elif p.device != self._device:
                raise ValueError(f"HipAdamW needs all parameters on one device ({self._device} and {p.device})")
        super().add_param_group(param_group)
        if len(self.param_groups) > 16:
            raise ValueError("HipAdamW supports at most 16 param groups")
        self._tables = None

    # ---- what the caller may read
    @property
    def norm_pass(self) -> bool:
        """True when step() measures the gradient norm (clipping or skipping is on)."""
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """0-dim fp32 device tensor: the global gradient norm of the last step() (0 when the norm pass is off)."""
        return self._state_block()[_W_NORM]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """0-dim int32 device tensor: the number of steps dropped for non-finite gradients so far."""
        return self._state_block().view(torch.int32)[_W_SKIPPED]

    def _state_block(self):
        n_groups = len(self.param_groups)
        words = int(_lib.lib().nbp_optim_state_bytes(n_groups)) // 4
        if words <= 0:
            raise _lib.NbpHipError("nbp_optim_state_bytes refused the param group count")
        if self._block is None or self._block.numel() < words:
            new = torch.zeros(words, dtype=torch.float32, device=self._device)
            if self._block is not None:          # a param group was added: the header (step, counters) carries over
                new[:_W_HEADER].copy_(self._block[:_W_HEADER])
            self._block = new
        return self._block

    # ---- tables
    def _build(self, groups, sig):
        """groups: per param group the list of parameters with a gradient.  Validates them, creates missing state, and builds the
        record table, the chunk table (one contiguous range per group) and the workspace of the norm pass."""
        L = _lib.lib()
        assert L.nbp_optim_desc_bytes() == _DESC.itemsize
        chunk = int(L.nbp_optim_chunk_elems())
        dev = self._device
        flat = [p for ps in groups for p in ps]
        fresh = [p for p in flat if len(self.state.get(p, ())) == 0]
        if fresh:
            if self._started or len(fresh) != len(flat):
                raise RuntimeError("HipAdamW keeps one step counter for all parameters: a parameter received its first gradient "
                                   "after the first step (or was missing from a loaded state)")
            steps = torch.zeros(len(flat), dtype=torch.float32, device=dev)
            for i, p in enumerate(flat):
                self.state[p] = {"step": steps[i], "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                 "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
        desc = np.zeros(len(flat), dtype=_DESC)
        chunks, ranges, step_views = [], [], []
        i = 0
        for ps in groups:
            c0 = sum(len(c) for c in chunks)
            for p in ps:
                g, st = p.grad, self.state[p]
                if g.is_sparse or g.layout is not torch.strided:
                    raise RuntimeError("HipAdamW does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != dev or g.shape != p.shape:
                    raise ValueError("HipAdamW needs fp32 gradients of the parameter's shape on its device")
                m, v = st["exp_avg"], st["exp_avg_sq"]
                for name, t in (("parameter", p), ("gradient", g), ("exp_avg", m), ("exp_avg_sq", v)):
                    if not t.is_contiguous():
                        raise ValueError(f"HipAdamW needs a contiguous {name}")
                    if t.data_ptr() % 4:
                        raise ValueError(f"HipAdamW needs a 4-byte aligned {name}")
                n = p.numel()
                if n < 1:
                    raise ValueError("HipAdamW cannot update an empty parameter")
                desc[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n)
                c = np.zeros((n + chunk - 1) // chunk, dtype=_CHUNK)
                c["first"] = np.arange(len(c), dtype=np.int64) * chunk
                c["tensor"] = i
                chunks.append(c)
                step_views.append(st["step"])
                i += 1
            ranges.append((c0, sum(len(c) for c in chunks) - c0))
        chunks = np.concatenate(chunks)
        # the per-parameter `step` scalars are the elements of ONE array, which the finalize launch writes as a whole
        base = step_views[0]._base
        if base is None or base.dtype != torch.float32 or base.dim() != 1 or any(s._base is not base for s in step_views):
            raise RuntimeError("HipAdamW: the step scalars of the state are not the optimizer's own array (state replaced by hand?)")
        n_chunks = len(chunks)
        self._tables = {
            "sig": sig, "n": len(flat), "desc_host": desc, "descs": _upload(desc, device=dev), "chunks": _upload(chunks, device=dev),
            "n_chunks": n_chunks, "ranges": ranges, "steps": base, "n_steps": base.numel(),
            "ws": torch.empty(max(int(L.nbp_optim_workspace_bytes(n_chunks)), 8), dtype=torch.uint8, device=dev),
            "keep": [(p, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in flat],
        }

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("HipAdamW.step() takes no closure")
        groups, sig = [], []
        for group in self.param_groups:
            ps = []
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    ps.append(p)
                    sig.append(p.data_ptr())
                    sig.append(g.data_ptr())
            groups.append(ps)
        if not sig:
            return None
        L = _lib.lib()
        dev = self._device
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                return self.step()
        block = self._state_block()
        tab = self._tables
        if tab is None or tab["sig"] != sig:
            if tab is not None and tab["sig"][0::2] == sig[0::2]:       # only gradients moved: refresh their addresses
                for ps in groups:
                    for p in ps:
                        g = p.grad
                        if g.layout is not torch.strided or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                            raise ValueError("HipAdamW needs dense contiguous fp32 gradients of the parameter's shape")
                tab["desc_host"]["g"] = sig[1::2]
                _upload(tab["desc_host"], dst=tab["descs"])
                tab["sig"] = sig
            else:
                self._build(groups, sig)
                tab = self._tables
        st = _lib.current_stream()
        descs, chunks = tab["descs"].data_ptr(), tab["chunks"].data_ptr()
        n_groups = len(self.param_groups)
        betas = (ctypes.c_double * (2 * n_groups))()
        for i, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("HipAdamW has no amsgrad or maximize form")
            betas[2 * i], betas[2 * i + 1] = group["betas"]
        ws = 0
        if self.norm_pass:
            ws = tab["ws"].data_ptr()
            _lib.check(L.nbp_grad_sqnorm_f32(descs, chunks, tab["n_chunks"], ws, tab["ws"].numel(), st), "grad_sqnorm")
        _lib.check(L.nbp_optim_finalize_f32(ws, tab["n_chunks"], self.max_grad_norm or 0.0, int(self.skip_nonfinite), betas, n_groups,
                                            block.data_ptr(), tab["steps"].data_ptr(), tab["n_steps"], st), "optim_finalize")
        for i, (group, (c0, nc)) in enumerate(zip(self.param_groups, tab["ranges"])):
            if nc:
                _lib.check(L.nbp_adamw_f32(descs, chunks + 16 * c0, nc, block.data_ptr(), i, float(group["lr"]), group["betas"][0],
                                           group["betas"][1], group["eps"], group["weight_decay"], st), "adamw")
        self._started = True
        return None

    # ---- state exchange with torch.optim.AdamW
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
                raise ValueError("HipAdamW has no amsgrad, maximize or differentiable form")
            if not group.get("decoupled_weight_decay", True):
                raise ValueError("the loaded state is Adam's (coupled weight decay), not AdamW's")
            group.update(foreach=None, capturable=False, fused=True, decoupled_weight_decay=True)    # what this state is shaped like
        self._tables = None
        held = [p for group in self.param_groups for p in group["params"] if len(self.state.get(p, ())) != 0]
        if not held:
            self._started = False
            self._state_block()[_W_STEP] = 0.0
            return
        values = {float(self.state[p]["step"]) for p in held}      # (a host read: loading a state is not the training loop)
        if len(values) != 1:
            raise ValueError(f"HipAdamW keeps one step counter for all parameters; the loaded state holds {sorted(values)}")
        step = values.pop()
        steps = torch.full((len(held),), step, dtype=torch.float32, device=self._device)
        for i, p in enumerate(held):
            st = self.state[p]
            if "max_exp_avg_sq" in st:
                raise ValueError("the loaded state is an amsgrad state")
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].to(device=self._device, dtype=torch.float32).contiguous()
                if st[k].shape != p.shape:
                    raise ValueError(f"{k} of the loaded state does not have its parameter's shape")
            st["step"] = steps[i]
        self._state_block()[_W_STEP] = step
        self._started = True


# ---------------------------------------------------------------------------------------------------------------- weight averaging
def check_ema_decay(decay) -> float:
    """An EMA decay is a number in [0, 1); anything else raises ValueError."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)) or not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"the EMA decay must be a number in [0, 1), not {decay!r}")
    return float(decay)


class TensorEMA:
    """The binding of nbp_ema_update_f32: ``shadow[i] <- d shadow[i] + (1 - d) live[i]`` over two lists of fp32 device tensors, one
    launch for all of them (plus the one-thread launch that counts the update).  The number of applied updates lives in a device
    block of this object; the kernel forms ``d`` from it (``min(decay, (1 + n) / (10 + n))`` with warm-up), so the host never reads it.

    The shadows keep their addresses for the life of the object; the addresses of the live tensors are compared at every update (one
    ``data_ptr()`` each) and the record table is refreshed with one small copy when one moved."""

    def __init__(self, live, shadow):
        live, shadow = list(live), list(shadow)
        if not live or len(live) != len(shadow):
            raise ValueError("TensorEMA needs two tensor lists of the same, non-zero length")
        for t in live + shadow:
            if not isinstance(t, torch.Tensor):
                raise TypeError("TensorEMA averages Tensors")
            if not t.is_cuda:
                raise RuntimeError("TensorEMA runs on the GPU only (no CPU fallback): a tensor lives on " + str(t.device))
        self._device = live[0].device
        for p, e in zip(live, shadow):
            self._validate(p, "live tensor")
            self._validate(e, "shadow tensor")
            if p.shape != e.shape:
                raise ValueError("TensorEMA: a shadow tensor does not have its live tensor's shape")
        self._live, self._shadow = live, shadow
        self._tables = None
        L = _lib.lib()
        assert L.nbp_ema_desc_bytes() == _EMA_DESC.itemsize
        self._block = torch.zeros(int(L.nbp_ema_state_bytes()) // 4, dtype=torch.int32, device=self._device)

    def _validate(self, t, name):
        if t.layout is not torch.strided or t.dtype != torch.float32:
            raise ValueError(f"TensorEMA averages dense fp32 tensors only (the kernel is fp32): a {name} is {t.dtype}")
        if t.device != self._device:
            raise ValueError(f"TensorEMA needs all tensors on one device ({self._device} and {t.device})")
        if not t.is_contiguous() or t.data_ptr() % 4:
            raise ValueError(f"TensorEMA needs a contiguous, 4-byte aligned {name}")
        if t.numel() < 1:
            raise ValueError(f"TensorEMA cannot average an empty {name}")

    @property
    def num_updates(self) -> torch.Tensor:
        """0-dim int32 device tensor (a view of the state block): the number of updates applied so far."""
        return self._block[0]

    def set_num_updates(self, n: int) -> None:
        self._block[0] = int(n)

    def _build(self, sig):
        chunk = int(_lib.lib().nbp_optim_chunk_elems())
        desc = np.zeros(len(self._live), dtype=_EMA_DESC)
        chunks = []
        for i, (p, e) in enumerate(zip(self._live, self._shadow)):
            n = p.numel()
            desc[i] = (p.data_ptr(), e.data_ptr(), n)
            c = np.zeros((n + chunk - 1) // chunk, dtype=_CHUNK)
            c["first"] = np.arange(len(c), dtype=np.int64) * chunk
            c["tensor"] = i
            chunks.append(c)
        chunks = np.concatenate(chunks)
        self._tables = {"sig": sig, "desc_host": desc, "descs": _upload(desc, device=self._device),
                        "chunks": _upload(chunks, device=self._device), "n_chunks": len(chunks)}

    @torch.no_grad()
    def update(self, decay, warmup=True, optimizer=None):
        """Enqueues one update on the current stream.  `optimizer`: a HipAdamW whose step() was enqueued before this call -- the
        update is dropped on the device when that step was (skip_nonfinite); anything else, or None: the update always applies."""
        decay = check_ema_decay(decay)
        dev = self._device
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                return self.update(decay, warmup, optimizer)
        gate = 0
        if isinstance(optimizer, HipAdamW):
            if optimizer._device != dev:
                raise ValueError(f"the optimizer lives on {optimizer._device}, the averaged tensors on {dev}")
            gate = optimizer._state_block().data_ptr()
        sig = [p.data_ptr() for p in self._live]
        tab = self._tables
        if tab is None:
            self._build(sig)
            tab = self._tables
        elif tab["sig"] != sig:                  # a live tensor moved (the shadows never do): refresh the addresses
            for p, e in zip(self._live, self._shadow):
                self._validate(p, "live tensor")
                if p.shape != e.shape:
                    raise ValueError("TensorEMA: a live tensor changed its shape")
            tab["desc_host"]["p"] = sig
            _upload(tab["desc_host"], dst=tab["descs"])
            tab["sig"] = sig
        _lib.check(_lib.lib().nbp_ema_update_f32(tab["descs"].data_ptr(), tab["chunks"].data_ptr(), tab["n_chunks"],
                                                 self._block.data_ptr(), gate, decay, int(bool(warmup)), _lib.current_stream()),
                   "ema_update")


class WeightEMA:
    """An exponential moving average of a module's weights, kept on the device (csrc/nbp_ema.hip).

    ``WeightEMA(module, decay, warmup=True)``: ``.module`` is the shadow -- a deep copy of `module` made here, in eval mode, with
    ``requires_grad=False`` and the same attributes (``conv_precision``).  Every parameter and every floating-point buffer (the
    BatchNorm running statistics) is averaged, as timm's ``ModelEmaV2`` and ``swa_utils.AveragedModel(use_buffers=True)`` do:
    ``e <- d e + (1 - d) p`` with ``d = min(decay, (1 + n) / (10 + n))`` after n applied updates (``warmup=False``: ``d = decay``).
    Integer buffers (``num_batches_tracked``) are copied from the live module when the shadow is next handed out.

    ``update(optimizer=None)`` enqueues one update on the current stream and never waits for the device.  Call it right after
    ``optimizer.step()``.  Given a ``HipAdamW``, a step that optimizer dropped on the device (``skip_nonfinite``) drops the update
    too: shadow and counter keep their bits.  Any other optimizer, or None: every update applies.

    The kernel writes the shadow's tensors without touching their version counters, on which the packed eval weights and the
    captured forward graphs of an ``NBP`` are keyed: ``update()`` therefore drops the shadow's pack (``invalidate_packed()``), and
    the next forward of ``.module`` packs the averaged weights.

    ``num_updates`` is a 0-dim int32 device tensor; ``state_dict()`` / ``load_state_dict()`` exchange ``{"decay", "warmup",
    "num_updates", "shadow"}`` (a host read of the counter: not the training loop), and a restored average continues bit for bit.
    There is no CPU path: a module off the GPU raises ``RuntimeError``."""

    def __init__(self, module, decay, warmup=True):
        self.decay = check_ema_decay(decay)
        self.warmup = bool(warmup)
        tensors = list(module.parameters()) + list(module.buffers())
        if not tensors:
            raise ValueError("WeightEMA: the module has no parameters or buffers")
        if any(not t.is_cuda for t in tensors):
            raise RuntimeError("WeightEMA runs on the GPU only (no CPU fallback): the module is not on the device")
        shadow = copy.deepcopy(module)
        shadow.eval()
        shadow.requires_grad_(False)
        live_t, shadow_t, self._copied = [], [], []
        for (_, p), (_, e) in zip(module.named_parameters(), shadow.named_parameters()):
            live_t.append(p)
            shadow_t.append(e)
        for (_, p), (_, e) in zip(module.named_buffers(), shadow.named_buffers()):
            if p.dtype.is_floating_point:
                live_t.append(p)
                shadow_t.append(e)
            else:
                self._copied.append((p, e))
        self._shadow = shadow
        self._set = TensorEMA(live_t, shadow_t)
        self._stale = False          # the integer buffers of the shadow are behind the live ones

    @property
    def module(self):
        if self._stale:
            with torch.no_grad():
                for src, dst in self._copied:
                    dst.copy_(src)
            self._stale = False
        return self._shadow

    @property
    def num_updates(self) -> torch.Tensor:
        return self._set.num_updates

    def _drop_pack(self):
        drop = getattr(self._shadow, "invalidate_packed", None)
        if drop is not None:
            drop()

    def update(self, optimizer=None):
        self._set.update(self.decay, self.warmup, optimizer)
        self._stale = True
        self._drop_pack()

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": int(self.num_updates.item()),
                "shadow": self.module.state_dict()}

    def load_state_dict(self, state):
        decay = check_ema_decay(state["decay"])
        n = int(state["num_updates"])
        if n < 0:
            raise ValueError(f"num_updates of the loaded state is {n}")
        self._shadow.load_state_dict(state["shadow"], strict=True)
        self.decay, self.warmup = decay, bool(state["warmup"])
        self._set.set_num_updates(n)
        self._stale = False
        self._drop_pack()
