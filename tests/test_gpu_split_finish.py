"""The launch that finishes a split-K sum (conv3x3_halo_h2_kernel<FIN>, csrc/nbp_split.hip): a sliced layer runs as two convolution
launches, the slices before the last and then the last one alone, whose epilogue adds the earlier partial sums in slice order -- its
own accumulators last, the reduce kernels' order -- and writes the layer.  Every output must be bit-identical to the reduce launch's.

NBP_SPLIT_FINISH (0 = the reduce launch, 1 = the planner's rule, 2 = every sliced launch) is read once per process and only under
NBP_TUNING=1, so one script runs in fresh child processes and the parent compares what they saved."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from hip_helpers import conv3x3_split, nhwc, pack_conv_split
from nextbestpath_amd import _lib

pytestmark = pytest.mark.gpu

# (B, H, W, C, N, split_k, relu): H x W is the output
CONV_CASES = [
    (1, 16, 32, 128, 64, 2, 1),        # 8-row tiles, 32 wide <32, 2, 2>
    (1, 16, 32, 128, 64, 3, 1),        # ... 8 chunks as 3 + 3 + 2: the finishing slice is the short one
    (2, 32, 32, 256, 128, 4, 1),       # ... batch stride, two channel blocks, three earlier slices
    (2, 32, 32, 256, 128, 4, 0),       # ... no ReLU, negative shifts
    (2, 16, 16, 256, 128, 2, 1),       # 8-row tiles, 16 wide <16, 1, 4>
    (2, 16, 16, 256, 128, 8, 1),       # ... seven earlier slices
    (2, 256, 256, 64, 64, 2, 1),       # 256 workgroups before split-K: full-height 16 x 32 x 64 <32, 4, 2>
    (1, 256, 256, 64, 128, 2, 1),      # full-height 8 x 32 x 128 <32, 2, 4>
    (64, 16, 16, 64, 128, 2, 1),       # 16 wide, 64 images (64 workgroups before split-K: the planner's 8-row form)
    (64, 16, 16, 64, 512, 2, 1),       # 16 wide, 256 workgroups before split-K: full-height 16 x 16 x 128 <16, 2, 4>
]
# (B, Hs, Ws, C, N, split_k): Hs x Ws is the low-resolution input
UP_CASES = [
    (1, 16, 32, 64, 64, 2),            # 8-row parity form, 32 wide
    (2, 16, 16, 64, 128, 2),           # 8-row parity form, 16 wide
    (1, 128, 256, 64, 64, 2),          # two column parities per workgroup <32, 2, 2, PH, ., P2>
    (64, 16, 16, 64, 128, 2),          # one parity per workgroup, 16 wide <16, 2, 4, PH>
]
FORWARDS = [(1, 256), (1, 128), (3, 64)]      # (1, 256): the encoder runs split-K with the pool behind it; grouped decoder launches

_SCRIPT = r"""
import os, sys, torch
root, dst = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import test_gpu_split_finish as T
torch.save(T.run_cases(), dst)
"""


def _normal(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _layer_inputs(C, N, relu):
    w = _normal(N, C, 3, 3, seed=3) * (2.0 / (9 * C)) ** 0.5
    scale = _normal(N, seed=4) * 0.2 + 1.0
    shift = _normal(N, seed=5) * 0.1 if relu else -(_normal(N, seed=5).abs() * 0.3 + 0.05)
    return w.cuda().contiguous(), scale.cuda(), shift.cuda()


def _upconv(x, w, N, scale, shift, relu, split_k, amax_out):
    """nbp_upconv3x3_split_f32 with the max-|out| slot (hip_helpers.upconv3x3_split does not pass one)."""
    L = _lib.lib()
    B, Hs, Ws, Cc = x.shape
    H, W = 2 * Hs, 2 * Ws
    planes = torch.zeros(4 * (Cc // 16) * 4 * 4 * N * 8, dtype=torch.int16, device=x.device)
    wamax = torch.zeros(1, dtype=torch.int32, device=x.device)
    st = _lib.current_stream()
    _lib.check(L.nbp_pack_upconv_weight_split(_lib.ptr(w), N, Cc, _lib.ptr(planes), _lib.ptr(wamax), st), "pack_upconv")
    out = torch.empty(B, H, W, N, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(L.nbp_conv_split_workspace_bytes(B, H, W, N, split_k), 256), dtype=torch.uint8, device=x.device)
    rc = L.nbp_upconv3x3_split_f32(_lib.ptr(x), Cc, B, H, W, _lib.ptr(planes), _lib.ptr(wamax), N, _lib.ptr(scale), _lib.ptr(shift),
                                   int(relu), _lib.ptr(out), None, _lib.ptr(amax_out), split_k, _lib.ptr(ws), ws.numel(), st)
    _lib.check(rc, "upconv3x3_split")
    return out


def run_cases():
    """Every case under the process's own switches -> {key: tensors on the host} (a child process's whole job)."""
    from nextbestpath_amd.networks import packing
    from nextbestpath_amd.utility.synthetic import make_count_maps, make_explorer_state_dict
    res = {}
    for case in CONV_CASES:
        B, H, W, Cc, N, sk, relu = case
        w, scale, shift = _layer_inputs(Cc, N, relu)
        x = nhwc(_normal(B, Cc, H, W, seed=1)).cuda()
        amax = torch.zeros(64, dtype=torch.int32, device="cuda")
        out = conv3x3_split(x, None, 0, pack_conv_split(w), N, scale, shift, bool(relu), sk, amax_out=amax)
        res[("conv",) + case] = (out.cpu(), amax.view(torch.float32).max().cpu())
    for case in UP_CASES:
        B, Hs, Ws, Cc, N, sk = case
        w, scale, shift = _layer_inputs(Cc, N, 1)
        x = nhwc(_normal(B, Cc, Hs, Ws, seed=1)).cuda()
        amax = torch.zeros(64, dtype=torch.int32, device="cuda")
        out = _upconv(x, w, N, scale, shift, 1, sk, amax)
        res[("up",) + case] = (out.cpu(), amax.view(torch.float32).max().cpu())
    packed = packing.pack_state_dict(make_explorer_state_dict(9), torch.device("cuda"), precision="fp32_split")
    for B, S in FORWARDS:
        o1, o2 = packing.forward_packed(packed, make_count_maps(B, S, seed=B).cuda())
        res[("fwd", B, S)] = (o1.cpu(), o2.cpu())
    torch.cuda.synchronize()
    res["knobs"] = _lib.effective_knobs()                        # the switches this process ran off their defaults
    return res


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("split_finish")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp / "cases.py"
    script.write_text(_SCRIPT)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("NBP_")}
    out = {}
    for tag, env in (("default", {}), ("reduce", {"NBP_TUNING": "1", "NBP_SPLIT_FINISH": "0"}),
                     ("finish", {"NBP_TUNING": "1", "NBP_SPLIT_FINISH": "2"}),
                     ("polluted", {"NBP_SPLIT_FINISH": "0", "NBP_SPLIT_FINISH_MIN_WGS": "1"})):      # no NBP_TUNING=1: not read
        subprocess.run([sys.executable, str(script), root, str(tmp / f"{tag}.pt")], check=True, env={**clean, **env}, timeout=300)
        out[tag] = torch.load(tmp / f"{tag}.pt")
        os.remove(tmp / f"{tag}.pt")
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CONV_CASES)
def test_finishing_launch_equals_the_reduce_launch_conv(runs, case):
    key = ("conv",) + case
    out, amax = runs["finish"][key]
    assert float(amax) == float(out.abs().max()) > 0.0           # max |out| over the 64 words, from the finishing epilogue
    if not case[6]:
        assert float(out.min()) < 0.0                            # (no ReLU: the case does hold negative outputs)
    assert _same(runs["finish"][key], runs["reduce"][key])


@pytest.mark.parametrize("case", UP_CASES)
def test_finishing_launch_equals_the_reduce_launch_upconv(runs, case):
    key = ("up",) + case
    out, amax = runs["finish"][key]
    assert float(amax) == float(out.abs().max()) > 0.0
    assert _same(runs["finish"][key], runs["reduce"][key])


@pytest.mark.parametrize("B,S", FORWARDS)
def test_finishing_launches_in_the_whole_forward(runs, B, S):
    """Grouped two-decoder launches and the pool offer (the pool rides in the finishing epilogue instead of the reduce kernel)."""
    key = ("fwd", B, S)
    assert _same(runs["finish"][key], runs["reduce"][key])
    assert _same(runs["default"][key], runs["reduce"][key])      # the rule's own choice: the same bits


def test_the_switch_is_read_only_under_the_opt_in(runs):
    assert runs["reduce"]["knobs"].get("NBP_SPLIT_FINISH") == "0" and runs["finish"]["knobs"].get("NBP_SPLIT_FINISH") == "2"
    assert runs["polluted"]["knobs"] == runs["default"]["knobs"] == {}
    keys = [k for k in runs["default"] if k != "knobs"]
    assert set(runs["polluted"]) == set(runs["default"]) and len(keys) == len(CONV_CASES) + len(UP_CASES) + len(FORWARDS)
    for key in keys:
        assert _same(runs["polluted"][key], runs["default"][key]), key


def test_planned_slice_count_given_explicitly(hip):
    """Under the default build a layer called with the planner's own slice count equals the layer called with split_k = 0."""
    B, H, W, Cc, N = 2, 32, 32, 512, 128
    sk = C.c_int(0)
    hip.nbp_conv_split_planned_workspace_bytes(B, H, W, Cc, N, 0, C.byref(sk))
    assert sk.value >= 2
    w, scale, shift = _layer_inputs(Cc, N, 1)
    x = nhwc(_normal(B, Cc, H, W, seed=1)).cuda()
    packed = pack_conv_split(w)
    a0, a1 = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(2))
    planned = conv3x3_split(x, None, 0, packed, N, scale, shift, True, 0, amax_out=a0)
    given = conv3x3_split(x, None, 0, packed, N, scale, shift, True, sk.value, amax_out=a1)
    assert torch.equal(planned, given)
    assert a0.view(torch.float32).max().item() == a1.view(torch.float32).max().item() == planned.abs().max().item()
