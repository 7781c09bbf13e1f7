"""NBP value network -- host-side mirror of the reference interface, HIP compute.

Reference: next_best_path/networks/nbp_model.py:64-173 (class ``NBP``: Attention U-Net
with one shared encoder and two decoders).  This module keeps the reference's *interface*:

* ``NBP(img_ch=5, output_ch1=8, output_ch2=1)``
* ``forward(x) -> (out1 [B,8,S/4,S/4] linear, out2 [B,1,S,S] sigmoid)``
* ``loss(pred1, target1, pred2, target2)`` (uncertainty weighted MSE + BCE, ref :162-173)
* the exact 327 ``state_dict`` keys (``Conv1.conv.0.weight`` ... ``Final2.0.bias``,
  ``log_vars``) so a reference checkpoint loads with ``strict=True``.

The arithmetic is NOT torch: ``forward`` hands raw device pointers to the hand written
gfx950 kernels in ``csrc/`` through the C ABI declared in ``include/nbp_hip.h``
(BN is applied as a per-channel scale/shift in the conv epilogue, upsample / concat /
attention gate are fused into the operand gather of the implicit-GEMM convolution).
There is no CPU fallback: a CPU tensor, or a missing ``libnbp_hip.so``, raises.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

# (name, kind, c_in, c_out) in reference construction order (nbp_model.py:70-108).
# kind: "block" = conv3x3-BN-ReLU x2 under attribute ``conv`` (ref :8-21)
#       "up"    = Upsample(x2 nearest)-conv3x3-BN-ReLU under attribute ``up`` (ref :23-34)
#       "att"   = attention gate W_g / W_x / psi (ref :36-62); c_out is F_int
_ENCODER = [("Conv1", None, 64), ("Conv2", 64, 128), ("Conv3", 128, 256),
            ("Conv4", 256, 512), ("Conv5", 512, 1024)]
_DEC1 = [(5, 1024, 512), (4, 512, 256)]
_DEC2 = [(5, 1024, 512), (4, 512, 256), (3, 256, 128), (2, 128, 64)]


def _c3(ci, co):
    return nn.Conv2d(ci, co, kernel_size=3, stride=1, padding=1, bias=True)


def _c1(ci, co):
    return nn.Conv2d(ci, co, kernel_size=1, stride=1, padding=0, bias=True)


# rocprofv3 --pmc serialises every dispatch to read its counters and aborts the queue on a graph replay ("AQL packet is malformed",
# observed on ROCm 7.2 / gfx950): under counter collection forward_static runs the same launches eagerly (bit-identical outputs)
_COUNTER_COLLECTION = os.environ.get("ROCPROF_COUNTER_COLLECTION", "") not in ("", "0", "False", "false")

class _Holder(nn.Module):
    """A module whose only child is an ``nn.Sequential`` registered under ``attr``.

    This reproduces the reference's parameter *names* (``<X>.conv.<i>.*``, ``<X>.up.<i>.*``)
    without reproducing its module code; the Sequential is a parameter container only --
    it is never called on the product path.
    """

    def __init__(self, attr: str, layers):
        super().__init__()
        setattr(self, attr, nn.Sequential(*layers))


def _double_conv(ci, co):
    return _Holder("conv", [_c3(ci, co), nn.BatchNorm2d(co), nn.ReLU(inplace=True),
                            _c3(co, co), nn.BatchNorm2d(co), nn.ReLU(inplace=True)])


def _up_conv(ci, co):
    return _Holder("up", [nn.Upsample(scale_factor=2), _c3(ci, co), nn.BatchNorm2d(co),
                          nn.ReLU(inplace=True)])


class _Gate(nn.Module):
    def __init__(self, f_g, f_l, f_int):
        super().__init__()
        self.W_g = nn.Sequential(_c1(f_g, f_int), nn.BatchNorm2d(f_int))
        self.W_x = nn.Sequential(_c1(f_l, f_int), nn.BatchNorm2d(f_int))
        self.psi = nn.Sequential(_c1(f_int, 1), nn.BatchNorm2d(1), nn.Sigmoid())
        self.relu = nn.ReLU(inplace=True)


_MAX_GRAPHS = 8          # captured forwards kept by NBP.forward_static (each owns a forward workspace)


class NBP(nn.Module):
    def __init__(self, img_ch: int = 5, output_ch1: int = 8, output_ch2: int = 1):
        super().__init__()
        if (img_ch, output_ch1, output_ch2) != (5, 8, 1):
            raise ValueError("the HIP path is built for the reference's NBP(5, 8, 1)")
        self.Maxpool = nn.MaxPool2d(kernel_size=2, stride=2)
        for name, ci, co in _ENCODER:
            setattr(self, name, _double_conv(img_ch if ci is None else ci, co))
        # decoder 1 (value map) -- registration order follows the reference so that
        # default-initialised weights draw the global RNG in the same order.
        for lvl, ci, co in _DEC1:
            setattr(self, f"Up{lvl}_1", _up_conv(ci, co))
            setattr(self, f"Att{lvl}_1", _Gate(co, co, co // 2))
            setattr(self, f"Up_conv{lvl}_1", _double_conv(ci, co))
        self.Final1 = _c1(256, output_ch1)
        for lvl, ci, co in _DEC2:
            setattr(self, f"Up{lvl}_2", _up_conv(ci, co))
            setattr(self, f"Att{lvl}_2", _Gate(co, co, co // 2))
            setattr(self, f"Up_conv{lvl}_2", _double_conv(ci, co))
        self.Final2 = nn.Sequential(_c1(64, output_ch2), nn.Sigmoid())
        self.log_vars = nn.Parameter(torch.zeros(2))
        self._packed = None          # opaque handle into libnbp_hip (eval-mode packed weights)
        self._graphs = {}            # forward_static: (input address, shape, pack) -> packing.ForwardGraph
        self._packed_key = None
        self._tensors = None
        # eval-mode arithmetic of the convolutions (tensors are fp32 in all but "bf16"):
        #   "fp32_split" (default) fp32 operands scaled by a per-tensor power of two and cut into two fp16 pieces, three exact
        #                fp16 MFMAs per product, fp32 accumulation: the accuracy of the fp32 pipe (measured against fp64) at
        #                5.3x its matrix rate;
        #   "fp32"       the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32);
        #   "bf16"       bf16 activations and weights (BASELINE configs[4]).
        # All but "bf16" meet the 1e-4 parity bar.  NBP_TUNING=1 NBP_CONV_PRECISION=... overrides the default (A/B measurements).
        self.conv_precision = _lib.tune("NBP_CONV_PRECISION", "fp32_split")
        # train-mode arithmetic of the convolutions the split kernels take (networks/training.py, read once per training forward):
        #   "fp32_split" (default) the eval path's three exact fp16 MFMAs per fp32 product;
        #   "fp16"       scaled fp16 mixed precision: each operand scaled by its tensor's power of two (max |x| in [2^14, 2^15))
        #                and rounded once to fp16, ONE MFMA per product, fp32 accumulation, fp32 epilogues / master weights / AdamW.
        # Eval mode (conv_precision) is not affected.
        self.train_precision = "fp32_split"
        # eval-mode symmetry ensemble (test-time augmentation, the inference half of the D4 training augmentation): None (default)
        # = the plain forward, same launches, same bits; a name of utility/augment.py::ENSEMBLES ("c2", "flips", "d4") or a sequence
        # of distinct op codes starting with 0 = every eval forward (forward, forward_static, the planner's packed calls) runs the
        # network on the moved copies of its input and returns the average of the outputs moved back (augment.ensemble_reference):
        # about n times the forward plus two small launches.  Training mode ignores it.
        self._symmetry_ensemble = None

    @property
    def symmetry_ensemble(self):
        return self.__dict__.get("_symmetry_ensemble")

    @symmetry_ensemble.setter
    def symmetry_ensemble(self, spec):
        from ..utility import augment
        self.__dict__["_symmetry_ensemble"] = augment.check_ensemble(spec)

    # ------------------------------------------------------------------ packing
    def _state_key(self):
        # cheap staleness check: storage pointers + in-place version counters of every
        # parameter / buffer (optimizer steps and load_state_dict bump the versions)
        if self._tensors is None:
            self._tensors = list(self.parameters()) + list(self.buffers())
        return tuple((t.data_ptr(), t._version) for t in self._tensors)

    def invalidate_packed(self):
        self._graphs = {}
        if self._packed is not None:
            self._packed.free()
        self._packed = None
        self._packed_key = None
        self._tensors = None

    def __getstate__(self):
        # copy.deepcopy / pickle: the pack handle and the captured graphs belong to THIS object (a copied handle would be freed
        # twice); the copy packs its own weights at its first eval forward
        state = dict(self.__dict__)
        state.update(_packed=None, _graphs={}, _packed_key=None, _tensors=None)
        return state

    def forward_static(self, x: torch.Tensor):
        """Eval forward on a PERSISTENT input tensor (a rollout's net_in): captured once per (tensor, weights) into a hipGraph and
        replayed (packing.ForwardGraph).  Returns the graph's own out1 / out2: ALIASED buffers, overwritten by the next call on
        the same x (Rollout.step consumes them before its next forward; any other caller must copy what it keeps).  A graph owns a
        forward workspace and keeps x alive, so only the most recently used few are kept (a fresh RolloutState brings a new
        net_in address).  Inputs a capture cannot take (not contiguous, not fp32) go through forward()."""
        if self.training or not x.is_cuda or _COUNTER_COLLECTION or not x.is_contiguous() or x.dtype != torch.float32:
            return self.forward(x)
        from . import packing
        packed = self._ensure_packed(x.device)
        key = (x.data_ptr(), tuple(x.shape), id(packed))
        g = self._graphs.pop(key, None)
        if g is None:
            while len(self._graphs) >= _MAX_GRAPHS:
                # least recently used first (dicts keep insertion order).  A replay of it may still be running on a stream the
                # caller is not on (Rollout.step replays on side streams): wait before its buffers and executable go (rare).
                torch.cuda.synchronize(x.device)
                self._graphs.pop(next(iter(self._graphs)))
            g = packing.ForwardGraph(packed, x)
        self._graphs[key] = g                                      # (re-inserted: most recently used last)
        return g()

    def _apply(self, fn, *a, **k):     # .to() / .cuda() / .float() replace storages
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    def _ensure_packed(self, device):
        key = (self._state_key(), str(device), self.conv_precision, self.symmetry_ensemble)
        if self._packed is None or key != self._packed_key:
            from . import packing
            self._graphs = {}            # captured forwards point into the pack that is being replaced
            if self._packed is not None:
                self._packed.free()
            self._packed = packing.pack_eval_weights(self, device)
            self._packed_key = key
        return self._packed

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError(
                "nextbestpath_amd.NBP.forward runs on MI355X only (got a CPU tensor); "
                "there is no CPU fallback -- the CPU checker lives in oracle/ and is test-only")
        if x.dim() != 4 or x.shape[1] != 5 or x.shape[2] != x.shape[3] or x.shape[2] % 16:
            raise ValueError(f"expected [B,5,S,S] with S % 16 == 0, got {tuple(x.shape)}")
        if self.training:
            from . import training
            return training.forward_train(self, x)
        from . import packing
        return packing.forward_eval(self, x)

    # ------------------------------------------------------------------ loss (ref :162-173)
    def loss(self, pred1, target1, pred2, target2):
        if pred1.is_cuda:
            from . import training
            return training.loss(self, pred1, target1, pred2, target2)
        s = self.log_vars
        l1 = F.mse_loss(pred1, target1) / (2.0 * torch.exp(2 * s[0])) + s[0]
        l2 = F.binary_cross_entropy(pred2, target2) / torch.exp(2 * s[1]) + s[1]
        return l1 + l2
