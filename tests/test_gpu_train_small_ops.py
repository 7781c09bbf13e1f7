"""The training step's streaming and reduction kernels (csrc/nbp_train.hip, everything that is not a convolution) against the
float64 restatements of tests/train_ops_reference.py, at the sizes where their loops wrap and their twins part:

  * T = 524,288 work items is the cap of an element-wise launch (2048 blocks of 256): every streaming kernel gets one case past
    it; the loss partials cap at 131,072 elements, sum_n at 8192 blocks, the 16-lanes-per-row kernels at 32,768 rows, the column
    reductions at 1024 workgroups (32,768 rows);
  * every kernel with a 16-byte twin runs both at one shape, and once with C % 4 == 0 on tensors that start 4 bytes past a
    16-byte boundary (the scalar fallback);
  * selects and copies are compared with torch.equal, single fp32 operations bit for bit with the float64 result rounded once,
    everything else against a bound derived from the number of rounded operations (given where it is asserted).

Outputs are pre-filled with NaN, so an element a kernel does not write fails the comparison.  Each test prints its observed worst
error next to the bound (pytest -s)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import train_ops_reference as R
from nextbestpath_amd import _lib
from nextbestpath_amd.networks import training as tr

pytestmark = pytest.mark.gpu
D = "cuda"
T = 524288                       # nbp_ew_grid: at most 2048 blocks x 256 threads per element-wise launch
ROWS16 = 32768                   # ... which is 32,768 rows for the kernels that put 16 lanes on a row
LOSS_CAP = 131072                # the loss partial sums: at most 512 blocks x 256 threads
M_BIG = 3 * 32768 + 17           # column reductions: blocks_for_rows caps at 1024 workgroups = 32,768 rows of 32
U, DENORM = R.U, R.DENORM
NAN = float("nan")
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, 1e30, -1e30, 1.0, -1.0]          # +-0, denormals, huge


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _close(got, want, rtol=2e-4, what=""):          # tests/test_gpu_training.py::_close
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    print(f"  {what}: err {err:.3e} = {err / max(ref, 1e-300):.2e} of max {ref:.3e} (allowed {rtol:.0e})")
    assert err <= rtol * ref + 1e-6, f"{what}: err {err:.3e} vs max {ref:.3e}"


def _with_specials(t, values=SPECIALS, shift=0):
    """t (flat view) with the special values written over its first and its last elements"""
    flat = t.view(-1)
    v = torch.tensor(values, dtype=t.dtype).roll(shift)
    k = min(len(v), flat.numel())
    flat[:k] = v[:k]
    if flat.numel() >= 2 * len(v):
        flat[-len(v):] = v
    return t


_ALIVE = []


@pytest.fixture(autouse=True)
def _device_tensors_live_as_long_as_the_test():
    """A tensor made in the argument list of an entry point (`_lib.ptr(_dev(x))`) would be freed as soon as its address is taken, and
    the caching allocator hands its block to the next allocation -- before the kernel has read it.  _dev keeps what it makes."""
    yield
    _ALIVE.clear()


def _dev(t, misalign=False):
    """t on the device; misalign: in a contiguous view that starts 4 bytes past a 16-byte boundary"""
    if not misalign:
        out = t.to(D).contiguous()
        assert out.data_ptr() % 16 == 0
    else:
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=D)
        out = buf[1:1 + t.numel()].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    _ALIVE.append(out)
    return out


def _out(*shape, misalign=False):
    """a NaN-filled output"""
    return _dev(torch.full(shape, NAN), misalign)


def _ok(rc):
    assert rc == 0, _lib._ERR.get(rc, rc)


def _st():
    return _lib.current_stream()


def _exact(got, want64, want32, what):
    """bit for bit the float64 result rounded once, and the same fp32 operation on the CPU"""
    got = got.detach().cpu()
    for want, why in ((R.round_f32(want64), "the float64 result rounded once"), (want32, "the fp32 operation")):
        bad = (got != want).view(-1).nonzero().view(-1)[:4].tolist()
        assert not bad, f"{what}: not {why} at {bad}: got {got.reshape(-1)[bad].tolist()}, want {want.reshape(-1)[bad].tolist()}"


def _bounded(got, want64, bound, what):
    err = (got.detach().cpu().double() - want64).abs()
    assert not torch.isnan(err).any(), f"{what}: NaN"
    slack = err / bound.clamp_min(1e-300) if torch.is_tensor(bound) else err / bound
    k = int(slack.argmax())
    print(f"  {what}: worst error {float(err.view(-1)[k]):.3e} = {float(slack.view(-1)[k]):.3f} of its bound")
    assert (err <= bound).all(), f"{what}: error {float(err.view(-1)[k]):.3e} is {float(slack.view(-1)[k]):.2f} x the bound (element {k})"


def _slot_max(slot):
    """the 64 words of a max-|.| slot reduced as the consumer reduces them: non-negative float bits, so an integer max"""
    assert int(slot.min()) >= 0
    return float(slot.max().reshape(1).view(torch.float32)[0])


def _past_cap(C, vec):
    """rows M with M C just past the launch cap: T scalar work items, or T float4s"""
    return -(-(4 * T if vec else T) // C) + 3


# ================================================================================================ element-wise, ops 0 - 5
def _ew_inputs(op, n):
    a, b = _rand(n, seed=100 + op) * 4, _rand(n, seed=200 + op)
    if op in (0, 4):
        _with_specials(a)
        _with_specials(b, shift=1)
    elif op == 5:
        _with_specials(a)
        b = torch.tensor([0.37])
    elif op == 1:                     # a = dy, b = y: +0, -0 and denormals of both signs decide the mask
        _with_specials(a, shift=2)
        _with_specials(b, [0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, 0.5, -0.5])
    elif op == 2:
        inf = float("inf")
        _with_specials(a, [0.0, -0.0, 17.0, -17.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, inf, -inf, 1e-40, 1e30, -1e30])
        b = None
    elif op == 3:                     # a = dy, b = y = a sigmoid's output in [0, 1]
        _with_specials(a)
        b = torch.sigmoid(b * 8)
        _with_specials(b, [0.0, 1.0, 1e-40, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -126, 0.25, 1.0, 0.0], shift=3)
    return a, b


def _ew_check(op, a, b, got, what):
    want = R.elementwise(op, a, b)
    if op in (0, 4, 5):
        _exact(got, want, R.elementwise_f32(op, a, b), what)
    elif op == 1:
        assert torch.equal(got.cpu(), R.round_f32(want)), what
    else:
        # op 2: expf within 1 ulp, one addition, one correctly rounded division; op 3: three rounded operations; <= 8 u |ref|
        # plus one denormal for results below the normal range
        if op == 2:
            ulps = ((got.cpu().double() - want).abs() / (want.abs() * 2 * U).clamp_min(DENORM))
            print(f"  {what}: sigmoid worst error {float(ulps.max()):.2f} ulp at a = {float(a[int(ulps.argmax())])}")
        _bounded(got, want, 8 * U * want.abs() + DENORM, what)


def _ew_run(op, a, b, misalign=False):
    ad, bd = _dev(a, misalign), (None if b is None else _dev(b, misalign and b.numel() > 1))
    out = _out(a.numel(), misalign=misalign)
    _ok(_lib.lib().nbp_elementwise_f32(op, _lib.ptr(ad), _lib.ptr(bd), a.numel(), _lib.ptr(out), _st()))
    return out


@pytest.mark.parametrize("n", [1, 3, 255, 257, T + 259, 4 * T + 1200])
@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_elementwise(hip, op, n):
    """T + 259 is odd: the scalar kernel with a partial second grid-stride pass; 4 T + 1200 the float4 kernel with one."""
    a, b = _ew_inputs(op, n)
    _ew_check(op, a, b, _ew_run(op, a, b), f"op {op} n {n}")


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_elementwise_on_misaligned_views_is_the_scalar_kernel(hip, op):
    """n % 4 == 0 on views that start at element 1 of a larger buffer: not the float4 kernel; and both twins at one shape."""
    n = 4 * 300
    a, b = _ew_inputs(op, n)
    scalar, vec = _ew_run(op, a, b, misalign=True), _ew_run(op, a, b)
    _ew_check(op, a, b, scalar, f"op {op} misaligned")
    _ew_check(op, a, b, vec, f"op {op} aligned")


# ================================================================================================ row scale, outer, copies
@pytest.mark.parametrize("C,M,misalign", [(1, 7, False), (6, 7, False), (64, 7, False), (1, _past_cap(1, False), False),
                                          (6, _past_cap(6, False), False), (64, _past_cap(64, True), False),
                                          (64, _past_cap(64, False), True), (64, 7, True)])
def test_rowscale(hip, C, M, misalign):
    x, s = _with_specials(_rand(M, C, seed=1)), _with_specials(_rand(M, seed=2), [0.0, 1.0, -0.0, 1e-40])
    out = _out(M, C, misalign=misalign)
    _ok(hip.nbp_rowscale_f32(_lib.ptr(_dev(x, misalign)), _lib.ptr(_dev(s)), M, C, _lib.ptr(out), _st()))
    _exact(out, R.rowscale(x, s), R.rowscale_f32(x, s), f"rowscale C {C} M {M}")


@pytest.mark.parametrize("C,M,zero", [(4, 7, False), (64, 7, False), (64, _past_cap(64, True), False), (64, 33, True)])
def test_rowscale_amax(hip, C, M, zero):
    """the 64 slot words (non-negative float bits, reduced with an integer max as the consumer does) hold max |out| exactly"""
    x, s = _rand(M, C, seed=3) * 3, _rand(M, seed=4)
    if zero:
        x.zero_()
    out, slot = _out(M, C), torch.zeros(64, dtype=torch.int32, device=D)
    _ok(hip.nbp_rowscale_amax_f32(_lib.ptr(_dev(x)), _lib.ptr(_dev(s)), M, C, _lib.ptr(out), _lib.ptr(slot), _st()))
    _exact(out, R.rowscale(x, s), R.rowscale_f32(x, s), "rowscale_amax")
    assert _slot_max(slot) == float(R.rowscale_f32(x, s).abs().max())
    assert bool(zero) == (int(slot.max()) == 0)


def test_rowscale_amax_refuses_what_its_float4_kernel_cannot_take(hip):
    """C % 4 != 0 and a misaligned tensor are refused before anything is launched: the output keeps its fill"""
    for C, mis in ((6, False), (64, True)):
        x, s = _rand(5, C, seed=5), _rand(5, seed=6)
        out, slot = _out(5, C), torch.zeros(64, dtype=torch.int32, device=D)
        rc = hip.nbp_rowscale_amax_f32(_lib.ptr(_dev(x, mis)), _lib.ptr(_dev(s)), 5, C, _lib.ptr(out), _lib.ptr(slot), _st())
        assert rc != 0
        assert bool(torch.isnan(out).all()) and int(slot.max()) == 0


@pytest.mark.parametrize("C,M,misalign", [(1, 7, False), (6, 7, False), (64, 7, False), (6, _past_cap(6, False), False),
                                          (64, 9, True)])
def test_outer(hip, C, M, misalign):
    s, w = _with_specials(_rand(M, seed=7), [0.0, -0.0, 1e-40, 1e30]), _rand(C, seed=8)
    out = _out(M, C, misalign=misalign)
    _ok(hip.nbp_outer_f32(_lib.ptr(_dev(s)), _lib.ptr(_dev(w)), M, C, _lib.ptr(out), _st()))
    _exact(out, R.outer(s, w), R.outer_f32(s, w), f"outer C {C} M {M}")


@pytest.mark.parametrize("Cin,c0,Cs,M,misalign", [(64, 0, 4, 7, False), (64, 4, 4, 7, False), (64, 60, 4, 7, False),
                                                  (64, 3, 5, 7, False), (8, 4, 4, T + 3, False),
                                                  (8, 3, 5, _past_cap(5, False), False), (128, 64, 64, 9, False),
                                                  (128, 64, 64, 9, True)])
def test_slice_channels(hip, Cin, c0, Cs, M, misalign):
    x = _with_specials(_rand(M, Cin, seed=9))
    out = _out(M, Cs, misalign=misalign)
    _ok(hip.nbp_slice_channels_f32(_lib.ptr(_dev(x, misalign)), M, Cin, c0, Cs, _lib.ptr(out), _st()))
    assert torch.equal(out.cpu(), R.slice_channels(x, c0, Cs))


@pytest.mark.parametrize("Cin,Cout,M", [(5, 64, 7), (64, 64, 7), (1, 6, 7), (6, 6, 7), (5, 64, _past_cap(64, False))])
def test_pad_channels(hip, Cin, Cout, M):
    x = _with_specials(_rand(M, Cin, seed=10))
    out = _out(M, Cout)
    _ok(hip.nbp_pad_channels_f32(_lib.ptr(_dev(x)), M, Cin, Cout, _lib.ptr(out), _st()))
    assert torch.equal(out.cpu(), R.pad_channels(x, Cout))


# ================================================================================================ 2x2 windows
@pytest.mark.parametrize("C,B,Hs,Ws,misalign", [(1, 2, 3, 2, False), (6, 2, 3, 2, False), (64, 2, 3, 2, False),
                                                (1, 1, 1025, 512, False), (64, 1, 129, 256, False), (64, 2, 3, 2, True)])
def test_sum2x2(hip, C, B, Hs, Ws, misalign):
    """1025 x 512 windows of one channel and 129 x 256 of 64 are just past T scalar / float4 work items"""
    dy = _with_specials(_rand(B, 2 * Hs, 2 * Ws, C, seed=11))
    out = _out(B, Hs, Ws, C, misalign=misalign)
    _ok(hip.nbp_sum2x2_f32(_lib.ptr(_dev(dy, misalign)), B, Hs, Ws, C, _lib.ptr(out), _st()))
    assert torch.equal(out.cpu(), R.sum2x2_f32(dy)), "not (a + b) + (c + d) in fp32"
    want, mag = R.sum2x2(dy)
    _bounded(out, want, 3 * U * mag + DENORM, f"sum2x2 C {C}")          # three additions, each within u of a partial sum <= mag


_NINF = float("-inf")
WINDOWS = [[1, 1, 1, 1], [0, 2, 2, 1], [_NINF] * 4, [NAN, 0, 0, 0], [0, NAN, 0, 0], [0, 0, NAN, 0], [0, 0, 0, NAN],
           [0, NAN, NAN, 5], [NAN, 0, 9, NAN], [NAN] * 4, [3, 3, 7, 7], [_NINF, _NINF, 0, 0]]


def _maxpool_input(B, H, W, C, seed):
    """floor(3 rand) (many ties) with the special windows laid over the first windows of every image, rotated by channel"""
    x = torch.floor(_rand(B, H, W, C, seed=seed) * 3)
    k = 0
    for b in range(B):
        for wy in range(min(H // 2, 3)):
            for wx in range(min(W // 2, 2)):
                for c in range(min(C, 5)):
                    x[b, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2, c] = torch.tensor(WINDOWS[(k + c) % len(WINDOWS)]).view(2, 2)
                k += 1
    return x


def _maxpool_backward_aten(x, dy):
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy.permute(0, 3, 1, 2))
    return xr.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("C,B,H,W,misalign", [(1, 12, 2, 2, False), (3, 12, 2, 2, False), (64, 12, 2, 2, False),
                                              (1, 2, 6, 4, False), (3, 2, 6, 4, False), (64, 2, 6, 4, False),
                                              (1, 1, 2050, 1024, False), (64, 1, 258, 512, False), (64, 2, 6, 4, True)])
def test_maxpool2_backward(hip, C, B, H, W, misalign):
    """ATen's CPU max_pool2d backward on the same fp32 input, bit for bit: all-equal windows, ties, -inf everywhere, a NaN at each of
    the four positions, two NaNs, four NaNs; dx is written everywhere (zeros included)."""
    x = _maxpool_input(B, H, W, C, seed=12)
    dy = _rand(B, H // 2, W // 2, C, seed=13) + 2.0
    dx = _out(B, H, W, C, misalign=misalign)
    _ok(hip.nbp_maxpool2_backward_f32(_lib.ptr(_dev(x, misalign)), _lib.ptr(_dev(dy, misalign)), B, H, W, C, _lib.ptr(dx), _st()))
    assert torch.equal(dx.cpu(), _maxpool_backward_aten(x, dy)), "not ATen's max_pool2d backward"
    assert torch.equal(dx.cpu(), R.maxpool2_backward(x, dy))


# ================================================================================================ 16 lanes per row
@pytest.mark.parametrize("C", [1, 5, 16, 64, 68])
@pytest.mark.parametrize("M", [1, 17, ROWS16 + 5])
def test_rowdot(hip, M, C):
    """a row = 16 fmaf chains of ceil(C / 16) terms and a four-level tree: <= (C / 16 + 6) u sum_c |a b|"""
    a, b, w = _rand(M, C, seed=14), _rand(M, C, seed=15), _rand(C, seed=16)
    for vec, bb in ((0, b), (1, w)):
        out = _out(M)
        _ok(hip.nbp_rowdot_f32(_lib.ptr(_dev(a)), _lib.ptr(_dev(bb)), vec, M, C, _lib.ptr(out), _st()))
        want, mag = R.rowdot(a, bb)
        _bounded(out, want, (C / 16 + 6) * U * mag, f"rowdot M {M} C {C} vec {vec}")


@pytest.mark.parametrize("C", [4, 64, 68])
@pytest.mark.parametrize("M", [1, 17, ROWS16 + 5])
def test_rowscale_backward(hip, M, C):
    """dy read in place as a channel slice (row stride ldy, offsets 0 and 64) of a joint gradient: dx = dy s exactly, ds within
    (C / 16 + 6) u sum_c |dy x|"""
    x, s = _rand(M, C, seed=17), _rand(M, seed=18)
    xd, sd = _dev(x), _dev(s)
    for ldy in (C, C + 64, 3 * C):
        joint = _rand(M, ldy, seed=19 + ldy)
        jd = _dev(joint)
        for off in (0, 64):
            if off + C > ldy:
                continue
            dy = joint[:, off:off + C]
            dx, ds = _out(M, C), _out(M)
            _ok(hip.nbp_rowscale_backward_f32(jd.data_ptr() + 4 * off, ldy, _lib.ptr(xd), _lib.ptr(sd), M, C, _lib.ptr(dx),
                                              _lib.ptr(ds), _st()))
            want_dx, want_ds, mag = R.rowscale_backward(dy, x, s)
            _exact(dx, want_dx, R.rowscale_f32(dy, s), f"rowscale_backward dx ldy {ldy} off {off}")
            _bounded(ds, want_ds, (C / 16 + 6) * U * mag, f"rowscale_backward ds M {M} C {C} ldy {ldy} off {off}")


@pytest.mark.parametrize("C,view,misalign", [(64, True, False), (64, False, False), (6, False, False), (64, False, True)])
def test_rowscale_function_dispatch(hip, C, view, misalign):
    """RowScaleFn: the amax route for aligned C % 4 == 0, the plain one otherwise; its backward on a slice view of a wider gradient
    (read in place), on a contiguous one, for C % 4 != 0 (row scale + row dot) and for an x that is not 16-byte aligned"""
    B, H, W = 2, 3, 5
    M = B * H * W
    x, s = _rand(B, H, W, C, seed=20), _rand(B, H, W, 1, seed=21)
    joint = _rand(B, H, W, C + 64, seed=22)
    dy = joint[..., 64:] if view else joint[..., :C].contiguous()
    xd, sd = _dev(x, misalign).requires_grad_(True), _dev(s).requires_grad_(True)
    out = tr.RowScaleFn.apply(xd, sd)
    gd = _dev(joint)[..., 64:] if view else _dev(dy)
    assert gd.is_contiguous() != view
    out.backward(gd)
    x2, s1, dy2 = x.view(M, C), s.view(M), dy.reshape(M, C)
    _exact(out.view(M, C), R.rowscale(x2, s1), R.rowscale_f32(x2, s1), "RowScaleFn out")
    slot = tr._noted(out, "amax")
    assert (slot is not None) == (C % 4 == 0 and not misalign)
    if slot is not None:
        assert _slot_max(slot) == float(R.rowscale_f32(x2, s1).abs().max())
    want_dx, want_ds, mag = R.rowscale_backward(dy2, x2, s1)
    _exact(xd.grad.view(M, C), want_dx, R.rowscale_f32(dy2, s1), "RowScaleFn dx")
    _bounded(sd.grad.view(M), want_ds, (C / 16 + 6) * U * mag, "RowScaleFn ds")


# ================================================================================================ sum_n, FanOutFn
def _sum_n_sources(n, M, C, seed, mix=True):
    """n sources [M, C] on the CPU and the device: contiguous tensors and channel slices of wider ones (row stride 2 C and 3 C)"""
    cpu, devs, lds = [], [], []
    for k in range(n):
        kind = k % 3 if mix else 0
        ld, off = ((C, 0), (2 * C, C), (3 * C, C))[kind]
        wide = _rand(M, ld, seed=seed + k)
        wd = _dev(wide)
        cpu.append(wide[:, off:off + C])
        devs.append((wd, wd.data_ptr() + 4 * off))
        lds.append(ld)
    return cpu, devs, lds


def _sum_n_call(hip, n, devs, lds, M, C, out):
    ptrs = (ctypes.c_void_p * max(n, 1))(*[p for _, p in devs[:n]])
    ldv = (ctypes.c_longlong * max(n, 1))(*lds[:n])
    return hip.nbp_sum_n_f32(n, ptrs, ldv, M, C, _lib.ptr(out), _st())


def _sum_n_check(out, cpu, what):
    want, mag = R.sum_n(cpu)
    assert torch.equal(out.cpu(), R.sum_n_f32(cpu)), f"{what}: not the fp32 sum left to right"
    if len(cpu) <= 2:
        assert torch.equal(out.cpu(), R.round_f32(want)), f"{what}: not the float64 sum rounded once"
    _bounded(out, want, (len(cpu) - 1) * U * mag + DENORM, what)         # n - 1 additions, each within u of a partial sum <= mag


@pytest.mark.parametrize("C", [4, 64, 192, 1024, 2048])
def test_sum_n(hip, C):
    """C = 192: 48 float4 columns leave 16 threads of a block idle; C > 1024: the column loop; M = 1, 7, 33 with the rows of a
    block and the two rows in flight: every tail.  n = 1 is a copy."""
    for M in (1, 7, 33):
        cpu, devs, lds = _sum_n_sources(8, M, C, seed=30 + M)
        for n in (1, 2, 3, 8):
            out = _out(M, C)
            _ok(_sum_n_call(hip, n, devs, lds, M, C, out))
            _sum_n_check(out, cpu[:n], f"sum_n n {n} M {M} C {C}")


def test_sum_n_past_the_block_cap(hip):
    """C = 1024, M = 16,384 + 3: 8192 blocks of one row, two rows in flight, three rows in a second pass"""
    M, C = 16384 + 3, 1024
    cpu, devs, lds = _sum_n_sources(3, M, C, seed=40, mix=False)
    out = _out(M, C)
    _ok(_sum_n_call(hip, 3, devs, lds, M, C, out))
    _sum_n_check(out, cpu, "sum_n wrap")


@pytest.mark.parametrize("n", [0, 9])
def test_sum_n_refuses_a_source_count_it_cannot_hold(hip, n):
    cpu, devs, lds = _sum_n_sources(9, 7, 64, seed=41)
    out = _out(7, 64)
    assert _sum_n_call(hip, n, devs, lds, 7, 64, out) != 0
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("C,route", [(64, "direct"), (64, "autograd"), (6, "direct"), (6, "autograd"), (192, "direct")])
def test_fan_out_function(hip, C, route):
    """FanOutFn.backward with three live gradients -- a contiguous one, a channel slice of a wider tensor (read in place), a slice
    that starts off a 16-byte boundary (copied) -- and, called directly, one None; C % 4 != 0 takes the torch adds."""
    shp = (2, 3, 5, C)
    g0, wide, odd = _rand(*shp, seed=50), _rand(2, 3, 5, 3 * C, seed=51), _rand(2, 3, 5, C + 4, seed=52)
    g1, g2 = wide[..., C:2 * C], odd[..., 1:C + 1]
    d0, d1, d2 = _dev(g0), _dev(wide)[..., C:2 * C], _dev(odd)[..., 1:C + 1]
    assert not d1.is_contiguous() and d2.data_ptr() % 16 != 0
    if route == "direct":
        got, none = tr.FanOutFn.backward(None, d0, None, d1, d2)
        assert none is None
        assert tr.FanOutFn.backward(None, None, None) == (None, None)
        assert tr.FanOutFn.backward(None, None, d1)[0] is d1
    else:
        x = torch.zeros(shp, device=D, requires_grad=True)
        outs = tr.FanOutFn.apply(x, 3)
        torch.autograd.backward(list(outs), [d0, d1, d2])
        got = x.grad
    cpu = [g.reshape(-1, C) for g in (g0, g1, g2)]
    assert got.shape == shp
    _sum_n_check(got.reshape(-1, C), cpu, f"FanOutFn C {C} {route}")


# ================================================================================================ losses
SATURATED = [(p, t) for t in (1.0, 0.0) for p in (0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 2.0 ** -126)]


def _loss_inputs(mode, n):
    if mode == 0:
        p, t = _rand(n, seed=60) * 3, _rand(n, seed=61)
        _with_specials(p, [0.0, -0.0, 1e-40, 30.0, -30.0, 1.0])
        _with_specials(t, [1.0, 1e-40, -0.0, 0.0, 30.0, 1.0])
        return p, t
    # BCE: interior p (p (1 - p) >= 2e-3, far from the gradient's 1e-12 clamp) with hard and soft targets, and a saturated block at
    # both ends (p (1 - p) <= 1e-30 or >= 5e-8: a factor 4 and more from the clamp on either side)
    p = torch.sigmoid(_rand(n, seed=62) * 6)
    t = torch.where(_rand(n, seed=63) > 0, (_rand(n, seed=64) > 0).float(), _rand(n, seed=65).abs())
    _with_specials(p, [q for q, _ in SATURATED])
    _with_specials(t, [q for _, q in SATURATED])
    pq = p.double() * (1.0 - p).double()
    assert ((pq < R.GRAD_CLAMP / 4) | (pq > R.GRAD_CLAMP * 4)).all()
    return p, t


def _loss_call(hip, mode, pd, td, coef, dp):
    acc = torch.full((1,), NAN, dtype=torch.float64, device=D)
    ws = torch.empty(512 * 8 + 256, dtype=torch.uint8, device=D)
    _ok(hip.nbp_loss_f32(mode, _lib.ptr(pd), _lib.ptr(td), pd.numel(), coef, _lib.ptr(acc), _lib.ptr(dp), _lib.ptr(ws),
                         ws.numel(), _st()))
    return acc


@pytest.mark.parametrize("n", [1, 255, LOSS_CAP + 77, T + 77])
@pytest.mark.parametrize("mode", [0, 1])
def test_loss(hip, mode, n):
    """Sum: fp32 terms (at most four rounded operations and a 1-ulp logf) accumulated in double: <= 8 u sum |term|.  Gradient: at
    most five rounded operations: <= 8 u |ref| + one denormal.  n past 131,072 wraps the partial sums, past T the gradient."""
    p, t = _loss_inputs(mode, n)
    pd, td = _dev(p), _dev(t)
    want, mag = R.loss_sum(mode, p, t)
    plain = _loss_call(hip, mode, pd, td, 1.0, None)                   # dp_or_null = NULL
    _bounded(plain, want.view(1), 8 * U * float(mag), f"loss sum mode {mode} n {n}")
    for coef in (1.0, 0.37):
        dp = _out(n)
        acc = _loss_call(hip, mode, pd, td, coef, dp)
        assert torch.equal(acc, plain)
        ref = R.loss_grad(mode, p, t, coef)
        _bounded(dp, ref, 8 * U * ref.abs() + DENORM, f"loss grad mode {mode} n {n} coef {coef}")
    # MeanLossFn: that sum divided by n, rounded to fp32; its backward takes the incoming gradient as the coefficient
    for coef in (1.0, 0.37):
        pg = pd.clone().requires_grad_(True)
        val = tr.MeanLossFn.apply(pg, td, mode)
        assert val.dtype == torch.float32 and val.shape == ()
        assert torch.equal(val.cpu().double(), (plain.cpu() / n).float().double().reshape(()))
        (val * coef).backward()
        ref = R.loss_grad(mode, p, t, coef)
        _bounded(pg.grad, ref, 8 * U * ref.abs() + DENORM, f"MeanLossFn grad mode {mode} n {n} coef {coef}")


# ================================================================================================ column reductions past the block cap
@pytest.mark.parametrize("C", [1, 6, 64])
def test_colsum_past_the_block_cap(hip, C):
    """M = 3 * 32,768 + 17: 1024 workgroups that each walk more than 32 rows.  Products and sums are carried in double and rounded
    once: <= 2 u sum_m |rows x|; two runs are bit-identical."""
    M = M_BIG
    x, rows = _rand(M, C, seed=70) + 0.25, _rand(M, seed=71)
    xd, rd = _dev(x), _dev(rows)
    ws = torch.empty(hip.nbp_colreduce_workspace_bytes(M, C), dtype=torch.uint8, device=D)
    for r_cpu, r_dev in ((None, None), (rows, rd)):
        outs = []
        for _ in range(2):
            ws.fill_(255)
            out = _out(C)
            _ok(hip.nbp_colsum_f32(_lib.ptr(xd), _lib.ptr(r_dev), M, C, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st()))
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        want, mag = R.colsum(x, r_cpu)
        _bounded(outs[0], want, 2 * U * mag, f"colsum C {C} rows {r_cpu is not None}")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [1, 6, 64])
def test_batchnorm_function_past_the_block_cap(hip, C, relu):
    """BNFn forward and backward at M = 3 * 32,768 + 17 against float64 autograd of F.batch_norm on the fp32 inputs (the tolerances
    of test_batchnorm_train_function); two runs are bit-identical."""
    M = M_BIG
    x = _rand(M, C, seed=72) * 2 + 0.3
    g, b = _rand(C, seed=73) * 0.3 + 1, _rand(C, seed=74) * 0.2
    rm, rv = _rand(C, seed=75) * 0.1, _rand(C, seed=76).abs() + 0.5
    gy = _rand(M, C, seed=77)
    y_ref, (dx_ref, dg_ref, db_ref), mean, var = R.batch_norm_train(x, g, b, relu, gy)
    runs = []
    for _ in range(2):
        xd, gd, bd = [_dev(t).requires_grad_(True) for t in (x.view(1, 1, M, C), g, b)]
        rmd, rvd = _dev(rm), _dev(rv)
        y = tr.BNFn.apply(xd, gd, bd, rmd, rvd, 1e-5, 0.1, relu)
        y.backward(_dev(gy.view(1, 1, M, C)))
        runs.append((y.detach(), xd.grad, gd.grad, bd.grad, rmd, rvd))
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    y, dx, dg, db, rmd, rvd = runs[0]
    _close(y.view(M, C), y_ref, what="y")
    _close(rmd, 0.9 * rm.double() + 0.1 * mean, what="running_mean")
    _close(rvd, 0.9 * rv.double() + 0.1 * var, what="running_var")
    _close(dx.view(M, C), dx_ref, rtol=5e-4, what="dx")
    _close(dg, dg_ref, what="dgamma")
    _close(db, db_ref, what="dbeta")


def test_gate_middle_function_past_the_block_cap(hip):
    """GateMidFn with F = 32 at M = 3 * 32,768 + 17 against float64 autograd of the unfused formula; two runs are bit-identical.
    The incoming gradient is zero on the few rows where BN_g + BN_x comes within 1e-5 of zero: there the sign of an fp32 sum of two
    fp32-rounded terms (error ~1e-7) is not the sign of the exact one, and a flipped ReLU mask is no error of the kernel."""
    M, Fi = M_BIG, 32
    assert tr._GATE_FUSE
    gp, xp = _rand(M, Fi, seed=80) * 2 + 0.3, _rand(M, Fi, seed=81) - 0.2
    gg, bg, gx, bx = _rand(Fi, seed=82) * 0.3 + 1, _rand(Fi, seed=83) * 0.2, _rand(Fi, seed=84) * 0.3 + 0.8, _rand(Fi, seed=85) * 0.2
    w, b, dp = _rand(1, Fi, 1, 1, seed=86), _rand(1, seed=87), _rand(M, seed=88)
    close_call = (R.gate_preactivation(gp, xp, gg, bg, gx, bx).abs() < 1e-5).any(1)
    assert int(close_call.sum()) < M // 100
    dp[close_call] = 0.0
    p_ref, grads_ref = R.gate_middle(gp, xp, gg, bg, gx, bx, w.view(Fi), b, dp)
    runs = []
    for _ in range(2):
        leaves = [_dev(t).requires_grad_(True) for t in (gp.view(1, 1, M, Fi), xp.view(1, 1, M, Fi), gg, bg, gx, bx, w, b)]
        bufs = [_dev(torch.zeros(Fi)), _dev(torch.ones(Fi)), _dev(torch.zeros(Fi)), _dev(torch.ones(Fi))]
        assert tr._gate_mid_ok(leaves[0], leaves[1])
        p = tr.GateMidFn.apply(leaves[0], leaves[1], leaves[2], leaves[3], bufs[0], bufs[1], 1e-5, 0.1, leaves[4], leaves[5],
                               bufs[2], bufs[3], 1e-5, 0.1, leaves[6], leaves[7])
        p.backward(_dev(dp.view(1, 1, M, 1)))
        runs.append([p.detach()] + [t.grad for t in leaves] + bufs)
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    got = runs[0]
    _close(got[0].view(M), p_ref, what="p")
    names = ("d g_pre", "d x_pre", "dgamma_g", "dbeta_g", "dgamma_x", "dbeta_x", "dw_psi", "db_psi")
    for nm, a, r in zip(names, got[1:9], grads_ref):
        _close(a.reshape(r.shape), r, rtol=5e-4 if nm.startswith("d ") else 2e-4, what=nm)
    _close(got[9], 0.1 * gp.double().mean(0), what="running_mean_g")
    _close(got[12], 0.9 + 0.1 * xp.double().var(0, unbiased=True), what="running_var_x")


# ================================================================================================ sparse value targets
MAP = (2, 8, 16, 16)
OUTSIDE = [[0, -1, 3, 3], [1, 8, 3, 3], [0, 2, -1, 3], [1, 2, 16, 3], [0, 2, 3, -1], [1, 2, 3, 16], [1, -1, -1, -1], [0, 8, 16, 16]]


def _coords(K):
    """K coordinates inside the map (K = 5000: drawn from 50 distinct cells), a block of them replaced by ones whose channel, row or
    column is -1 or the extent (the batch index stays inside [0, B): the kernels do not check it)"""
    g = torch.Generator().manual_seed(90 + K)
    B, C, H, W = MAP
    cells = torch.stack([torch.randint(0, e, (50 if K == 5000 else max(K, 1),), generator=g) for e in MAP], 1)
    c = cells[torch.randint(0, cells.shape[0], (K,), generator=g)] if K == 5000 else cells[:K]
    if K >= 257:
        c[100:100 + len(OUTSIDE)] = torch.tensor(OUTSIDE)
        c[-1] = torch.tensor(OUTSIDE[1])
    return c.contiguous()


@pytest.mark.parametrize("K", [0, 1, 257, 5000])
def test_gather_and_scatter_values(hip, K):
    """K > 256 needs a second block; coordinates outside the map read as 0 and scatter nothing (both kernels check channel, row and
    column before they form an address); duplicates accumulate with float atomics in any order: a cell hit d times is within
    d u sum |its terms|."""
    o1, coords, dpred = _rand(*MAP, seed=91), _coords(K), _rand(K, seed=92).abs() + 0.5
    od, cd = _dev(o1), coords.to(D)
    pred = _out(K)
    _ok(hip.nbp_gather_values_f32(_lib.ptr(od), _lib.ptr(cd), K, MAP[1], MAP[2], MAP[3], _lib.ptr(pred), _st()))
    want = R.gather_values(o1, coords)
    assert torch.equal(pred.cpu(), want)
    if K >= 257:
        assert int((~R.coords_in_range(coords, MAP)).sum()) == len(OUTSIDE) + 1 and float(want[100:108].abs().max()) == 0.0
    d1 = torch.zeros(MAP, device=D)
    _ok(hip.nbp_scatter_values_f32(_lib.ptr(_dev(dpred)), _lib.ptr(cd), K, MAP[1], MAP[2], MAP[3], _lib.ptr(d1), _st()))
    ref, mag, mult = R.scatter_values(dpred, coords, MAP)
    assert torch.equal(d1.cpu() != 0, mult > 0)                     # nothing outside the addressed cells (dpred >= 0.5 > 0)
    _bounded(d1, ref, mult * U * mag + DENORM, f"scatter K {K} (largest multiplicity {int(mult.max())})")
    if K == 5000:
        assert int((mult > 0).sum()) <= 50 and int(mult.max()) > 50
    # the Function: the same gather, and the scatter as its backward
    og = od.clone().requires_grad_(True)
    pf = tr.GatherValuesFn.apply(og, cd)
    assert torch.equal(pf.cpu(), want)
    if K:
        pf.backward(_dev(dpred))
        _bounded(og.grad, ref, mult * U * mag + DENORM, f"GatherValuesFn backward K {K}")
