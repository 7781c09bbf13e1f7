"""The frontier policy and the information-gain policy as objects that stand where the NBP network stands in a rollout.

Rollout and MultiRollout ask the object they were given for the planner's two inputs.  A network gets the five-channel input
`net_in`; an object with `wants_maps6` gets the six-channel map stack instead (`forward_maps`), because only the stack knows seen
free space (utility/frontier.py, utility/infogain.py).  Everything downstream -- obstacle fusion, candidate scoring, the edge mask, the host search, the
heading choice -- is the network's path unchanged.
"""
from __future__ import annotations

import torch

from .. import _lib
from ..utility import frontier as frontier_options
from ..utility import hipops
from ..utility import infogain as infogain_options


class FrontierPolicy:
    """forward_maps(maps6 [B,6,S,S]) -> (out1 [B,8,V,V], out2 [B,1,S,S]) on the current stream, no host synchronisation.  The
    outputs are buffers of the policy, one pair per (batch size, grid, device, stream): a later call of the same shape on the same
    stream overwrites them in stream order, as a replayed forward graph overwrites its outputs."""

    wants_maps6 = True
    training = False
    _options = frontier_options
    _kernel = staticmethod(hipops.frontier_policy)

    def __init__(self, spec=None):
        spec = self._options.option_spec(self._options.NAME if spec is None else spec)
        if spec is None:
            raise ValueError(f"{type(self).__name__}: a {self._options.NAME} spec is needed ('nbp' / None means the network)")
        self.options = spec
        self._out = {}
        self.calls = 0

    @property
    def symmetry_ensemble(self):
        return None

    @symmetry_ensemble.setter
    def symmetry_ensemble(self, spec):
        if spec is not None:
            raise ValueError(f"a policy takes no symmetry ensemble (the {self._options.NAME} policy is exactly D4-equivariant)")

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def _kernel_options(self):
        o = self.options
        return {"radius": o["radius"], "dilate": o["dilate"], "unknown": o["unknown"], "distance_penalty": o["distance_penalty"]}

    def forward_maps(self, maps6):
        B, S = maps6.shape[0], maps6.shape[-1]
        key = (B, S, maps6.device.index, _lib.current_stream())
        out = self._out.get(key)
        if out is None:
            V = S // 4
            out = self._out[key] = (torch.empty(B, 8, V, V, dtype=torch.float32, device=maps6.device),
                                    torch.empty(B, 1, S, S, dtype=torch.float32, device=maps6.device))
        self.calls += 1
        return self._kernel(maps6, out=out, **self._kernel_options())

    def __call__(self, net_in):
        raise TypeError(f"{type(self).__name__} reads the map stack: call forward_maps(maps6), not the network input")


class InfoGainPolicy(FrontierPolicy):
    """The same object around hipops.infogain_policy (utility/infogain.py: the unknown pixels a camera on the cell would see)."""

    _options = infogain_options
    _kernel = staticmethod(hipops.infogain_policy)


POLICIES = {frontier_options.NAME: FrontierPolicy, infogain_options.NAME: InfoGainPolicy}


def make_policy(spec):
    """The planning option `policy` -> None (the network), a FrontierPolicy or an InfoGainPolicy, by the spec's name.  ValueError on
    anything the named policy's option_spec refuses, and on any other name."""
    name = spec if isinstance(spec, str) else spec.get("name") if isinstance(spec, dict) else None
    if isinstance(name, str) and name in POLICIES:
        return POLICIES[name](spec)
    if isinstance(name, str) and name != "nbp":
        raise ValueError(f"policy: unknown policy {name!r} (known: 'nbp', " + ", ".join(repr(k) for k in POLICIES) + ")")
    if frontier_options.option_spec(spec) is not None:       # None, "nbp", {"name": "nbp"} -> the network; anything else raises
        raise ValueError("policy: not a policy spec")
    return None
