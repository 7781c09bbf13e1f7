"""tests/train_ops_reference.py without a GPU: each float64 restatement against torch's own float64 autograd or ATen operation on
small random inputs, so that what the GPU tests hold the kernels to is pinned by something other than itself."""
import pytest
import torch
import torch.nn.functional as F

import train_ops_reference as R


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def _same(got, want, tol=1e-13):
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_elementwise_ops_against_autograd(op):
    a, b = _rand(37, seed=1) * 4, _rand(37, seed=2)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    if op == 0:
        _same(R.elementwise(0, a, b), F.relu(a64 + b64).detach())
        assert torch.equal(R.elementwise_f32(0, a, b), F.relu(a + b))
    elif op == 1:                                   # the backward of relu: dy where the OUTPUT y is positive
        y = F.relu(b64)
        y.backward(a.double())
        _same(R.elementwise(1, a, y.detach().float()), b64.grad)
        zeros = torch.tensor([0.0, -0.0, 1e-45, -1e-45])
        assert R.elementwise(1, torch.ones(4), zeros).tolist() == [0.0, 0.0, 1.0, 0.0]
    elif op == 2:
        _same(R.elementwise(2, a), torch.sigmoid(a64).detach())
        edge = torch.tensor([0.0, -104.0, 104.0, float("inf"), float("-inf")])
        assert R.elementwise(2, edge).tolist()[0] == 0.5 and R.elementwise(2, edge).tolist()[2:] == [1.0, 1.0, 0.0]
        assert 0.0 < float(R.elementwise(2, edge)[1]) < R.DENORM
    elif op == 3:                                   # the backward of sigmoid from its OUTPUT y
        y = torch.sigmoid(a64)
        y.backward(b.double())
        _same(R.elementwise(3, b, y.detach().float()), (b.double() * R.d(y.detach().float()) * (1 - R.d(y.detach().float()))))
        _same(R.elementwise(3, b, y.detach().float()), a64.grad, tol=1e-6)      # (y went through fp32)
    elif op == 4:
        _same(R.elementwise(4, a, b), (a64 + b64).detach())
        assert torch.equal(R.elementwise_f32(4, a, b), a + b)
    else:
        _same(R.elementwise(5, a, b), (a64 + b64[0]).detach())
        assert torch.equal(R.elementwise_f32(5, a, b), a + b[0])


@pytest.mark.parametrize("C", [1, 5, 68])
def test_row_and_column_pieces_against_autograd(C):
    M = 11
    x, s, dy, w = _rand(M, C, seed=3), _rand(M, seed=4), _rand(M, C, seed=5), _rand(C, seed=6)
    x64, s64 = x.double().requires_grad_(True), s.double().requires_grad_(True)
    out = x64 * s64[:, None]
    _same(R.rowscale(x, s), out.detach())
    out.backward(dy.double())
    dx, ds, mag = R.rowscale_backward(dy, x, s)
    _same(dx, x64.grad)
    _same(ds, s64.grad)
    _same(mag, (dy.double() * x.double()).abs().sum(1))
    assert torch.equal(R.rowscale_f32(x, s), x * s.view(M, 1))
    _same(R.outer(s, w), torch.outer(s.double(), w.double()))
    assert torch.equal(R.outer_f32(s, w), torch.outer(s, w))
    _same(R.rowdot(x, dy)[0], torch.einsum("mc,mc->m", x.double(), dy.double()))
    _same(R.rowdot(x, w)[0], x.double() @ w.double())
    _same(R.rowdot(x, w)[1], x.double().abs() @ w.double().abs())
    _same(R.colsum(x)[0], x.double().sum(0))
    _same(R.colsum(x, s)[0], s.double() @ x.double())
    _same(R.colsum(x, s)[1], s.double().abs() @ x.double().abs())


def test_sum_n_is_the_gradient_of_a_fan_out():
    srcs = [_rand(7, 12, seed=10 + k) for k in range(5)]
    x = torch.zeros(7, 12, dtype=torch.float64, requires_grad=True)
    sum((x * 1.0 * g.double()).sum() for g in srcs).backward()           # five consumers of x
    _same(R.sum_n(srcs)[0], x.grad)
    _same(R.sum_n(srcs)[1], sum(g.double().abs() for g in srcs))
    assert torch.equal(R.sum_n_f32(srcs), (((srcs[0] + srcs[1]) + srcs[2]) + srcs[3]) + srcs[4])
    assert torch.equal(R.sum_n_f32(srcs[:1]), srcs[0])


def test_slice_and_pad_channels():
    x = _rand(9, 8, seed=20)
    assert torch.equal(R.slice_channels(x, 3, 5), x[:, 3:8])
    assert torch.equal(R.pad_channels(x, 8), x)
    assert torch.equal(R.pad_channels(x[:, :5].contiguous(), 64), F.pad(x[:, :5], (0, 59)))


@pytest.mark.parametrize("C", [1, 3])
def test_sum2x2_is_the_backward_of_nearest_upsampling(C):
    dy = _rand(2, 6, 4, C, seed=30)
    small = torch.zeros(2, C, 3, 2, dtype=torch.float64, requires_grad=True)
    F.interpolate(small, scale_factor=2, mode="nearest").backward(dy.double().permute(0, 3, 1, 2))
    _same(R.sum2x2(dy)[0], small.grad.permute(0, 2, 3, 1))
    assert float((R.sum2x2_f32(dy).double() - R.sum2x2(dy)[0]).abs().max()) <= 3 * R.U * float(R.sum2x2(dy)[1].max())
    assert (R.sum2x2(dy)[1] >= R.sum2x2(dy)[0].abs()).all()


def _maxpool_backward_aten(x, dy):
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy.permute(0, 3, 1, 2))
    return xr.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_maxpool_backward_rule_against_aten(dtype):
    """Ties (floor of 3 rand), all-equal windows, -inf windows and NaNs at every position: ATen's CPU max_pool2d backward sends
    the gradient to the first maximum in scan order, and a NaN takes over from whatever came before it (the last NaN wins)."""
    nan, ninf = float("nan"), float("-inf")
    x = torch.floor(_rand(2, 6, 8, 3, seed=40) * 3).to(dtype)
    wins = [[1, 1, 1, 1], [0, 2, 2, 1], [ninf] * 4, [nan, 0, 0, 0], [0, nan, 0, 0], [0, 0, nan, 0], [0, 0, 0, nan],
            [0, nan, nan, 5], [nan, nan, nan, nan], [3, nan, 7, ninf], [ninf, ninf, 0, 0]]
    for k, wv in enumerate(wins):
        y0, x0 = 2 * (k // 4), 2 * (k % 4)
        x[0, y0:y0 + 2, x0:x0 + 2, 1] = torch.tensor(wv, dtype=dtype).view(2, 2)
    dy = (_rand(2, 3, 4, 3, seed=41) + 2).to(dtype)
    got = R.maxpool2_backward(x, dy)
    assert torch.equal(got, _maxpool_backward_aten(x, dy))
    assert int((got != 0).sum()) == dy.numel()                   # exactly one element per window


def test_gather_and_scatter_against_index_put():
    o1 = _rand(2, 8, 6, 5, seed=50)
    g = torch.Generator().manual_seed(51)
    coords = torch.stack([torch.randint(0, 2, (300,), generator=g), torch.randint(0, 8, (300,), generator=g),
                          torch.randint(0, 2, (300,), generator=g), torch.randint(0, 3, (300,), generator=g)], 1)     # 12 cells x 2 x 8
    dpred = _rand(300, seed=52)
    o64 = o1.double().requires_grad_(True)
    pred = o64[coords[:, 0], coords[:, 1], coords[:, 2], coords[:, 3]]
    assert torch.equal(R.gather_values(o1, coords).double(), pred.detach())
    pred.backward(dpred.double())
    out, mag, mult = R.scatter_values(dpred, coords, o1.shape)
    _same(out, o64.grad)
    want = torch.zeros(o1.shape, dtype=torch.float64).index_put_(tuple(coords.t()), dpred.double(), accumulate=True)
    _same(out, want)
    assert float(mult.sum()) == 300 and float(mult.max()) > 1 and (mag >= out.abs() - 1e-15).all()
    # coordinates outside the map: read as 0, add nothing
    bad = torch.tensor([[0, -1, 0, 0], [0, 8, 0, 0], [1, 0, -1, 0], [1, 0, 6, 0], [0, 0, 0, -1], [0, 0, 0, 5], [1, 7, 5, 4]])
    assert R.coords_in_range(bad, o1.shape).tolist() == [False] * 6 + [True]
    assert R.gather_values(o1, bad).tolist() == [0.0] * 6 + [float(o1[1, 7, 5, 4])]
    out, _, mult = R.scatter_values(torch.ones(7), bad, o1.shape)
    assert float(out.sum()) == 1.0 and float(out[1, 7, 5, 4]) == 1.0 and float(mult.sum()) == 1.0


@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_losses_against_torch(coef):
    c32 = float(torch.tensor(coef, dtype=torch.float32))
    p, t = _rand(41, seed=60), _rand(41, seed=61)
    p64 = p.double().requires_grad_(True)
    loss = F.mse_loss(p64, t.double())
    (loss * c32).backward()
    s, mag = R.loss_sum(0, p, t)
    _same(s / 41, loss.detach())
    assert float(mag) == float(s)
    _same(R.loss_grad(0, p, t, coef), p64.grad)
    # BCE in the interior (soft and hard targets), where neither clamp binds and 1 - p in fp32 is 1 - p to 2^-24
    p = torch.sigmoid(_rand(41, seed=62) * 4)
    t = torch.cat([(_rand(20, seed=63) > 0).float(), _rand(21, seed=64).abs()])
    p64 = p.double().requires_grad_(True)
    loss = F.binary_cross_entropy(p64, t.double())
    (loss * c32).backward()
    s, mag = R.loss_sum(1, p, t)
    _same(s / 41, loss.detach(), tol=1e-6)
    _same(R.loss_grad(1, p, t, coef), p64.grad, tol=1e-6)
    assert float(mag) == float(s)


def test_bce_at_the_clamps():
    """p exactly 0 or 1: torch clamps the logarithm at -100 (the term is 100 or 0); the gradient divides by max(p (1-p), 1e-12)."""
    p = torch.tensor([0.0, 0.0, 1.0, 1.0])
    t = torch.tensor([0.0, 1.0, 0.0, 1.0])
    assert R.loss_terms(1, p, t).tolist() == [0.0, 100.0, 100.0, 0.0]
    want = F.binary_cross_entropy(p.double(), t.double(), reduction="none")
    _same(R.loss_terms(1, p, t), want)
    p64 = p.double().requires_grad_(True)
    F.binary_cross_entropy(p64, t.double()).backward()
    _same(R.loss_grad(1, p, t), p64.grad, tol=1e-6)
    assert R.loss_grad(1, p, t).tolist() == [0.0, -1.0 / R.GRAD_CLAMP / 4, 1.0 / R.GRAD_CLAMP / 4, 0.0]
    # below 2^-25 the fp32 1 - p is 1: the (1 - t) term is exactly 0, log p is not clamped
    tiny = torch.tensor([1e-30, 2.0 ** -126])
    terms = R.loss_terms(1, tiny, torch.tensor([0.0, 1.0]))
    assert float(terms[0]) == 0.0 and abs(float(terms[1]) - 126 * 0.6931471805599453) < 1e-12


@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_restatement(relu):
    """batch_norm_train is F.batch_norm's autograd re-laid over [M, C] rows: against the written-out formulas."""
    M, C = 53, 6
    x, g, b, dy = _rand(M, C, seed=70) * 2 + 0.3, _rand(C, seed=71) * 0.3 + 1, _rand(C, seed=72) * 0.2, _rand(M, C, seed=73)
    y, (dx, dg, db), mean, var = R.batch_norm_train(x, g, b, relu, dy)
    x64, dz = x.double(), dy.double().clone()
    mu, v = x64.mean(0), x64.var(0, unbiased=False)
    xhat = (x64 - mu) / torch.sqrt(v + 1e-5)
    yy = xhat * g.double() + b.double()
    if relu:
        dz[~(yy > 0)] = 0
        yy = yy.clamp_min(0)
    _same(y, yy, tol=1e-12)
    _same(db, dz.sum(0), tol=1e-12)
    _same(dg, (dz * xhat).sum(0), tol=1e-12)
    _same(dx, g.double() / torch.sqrt(v + 1e-5) * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0)), tol=1e-12)
    _same(mean, mu)
    _same(var, v * M / (M - 1), tol=1e-12)


def test_gate_middle_restatement():
    M, Fi = 29, 8
    gp, xp = _rand(M, Fi, seed=80), _rand(M, Fi, seed=81)
    gg, bg, gx, bx = [_rand(Fi, seed=82 + k) * 0.3 + (1 if k % 2 == 0 else 0) for k in range(4)]
    w, b, dp = _rand(Fi, seed=86), _rand(1, seed=87), _rand(M, seed=88)
    p, grads = R.gate_middle(gp, xp, gg, bg, gx, bx, w, b, dp)
    ones = torch.ones(M, Fi)
    g1 = R.batch_norm_train(gp, gg, bg, False, ones)[0]
    x1 = R.batch_norm_train(xp, gx, bx, False, ones)[0]
    q = (g1 + x1).clamp_min(0)
    _same(p, q @ w.double() + b.double(), tol=1e-12)
    dq = torch.where(q > 0, torch.outer(dp.double(), w.double()), torch.zeros_like(q))
    _same(grads[0], R.batch_norm_train(gp, gg, bg, False, dq.float())[1][0], tol=1e-6)
    _same(grads[6], q.t() @ dp.double(), tol=1e-12)
    _same(grads[7], dp.double().sum().view(1), tol=1e-12)
