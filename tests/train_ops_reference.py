"""Float64 restatements of the training step's small operations (csrc/nbp_train.hip: the streaming and reduction kernels
behind nbp_elementwise_f32 ... nbp_loss_f32), in plain torch on the CPU.

Every function takes the kernel's fp32 inputs (CPU tensors) and the semantics its entry point documents, and returns float64.
Nothing here imports the package or touches a GPU: tests/test_train_ops_host.py pins these functions to torch's own float64
autograd / ATen operations, tests/test_gpu_train_small_ops.py holds the kernels to them.  Activations are NHWC, [M, C] with
M = B*H*W.  The `*_f32` functions restate an operation in fp32 in the kernel's documented ORDER of operations (what a
bit-for-bit comparison is made against); `round_f32` is "rounded once to fp32".
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24              # unit roundoff of fp32
DENORM = 2.0 ** -149        # the smallest positive fp32 number
LOG_CLAMP = -100.0          # BCE: log is clamped here (torch.nn.functional.binary_cross_entropy)
GRAD_CLAMP = float(torch.tensor(1e-12, dtype=torch.float32))     # BCE gradient: p (1 - p) is clamped here (the kernel's 1e-12f)


def d(t):
    return t.detach().to(torch.float64)


def round_f32(t):
    return t.to(torch.float32)


# ---------------------------------------------------------------------------------------------- element-wise, ops 0 - 5
def elementwise(op, a, b=None):
    """op 0: relu(a + b); 1: a where b > 0 else 0; 2: sigmoid(a); 3: a b (1 - b); 4: a + b; 5: a + b[0]."""
    a64 = d(a)
    if op == 0:
        return torch.clamp_min(a64 + d(b), 0.0)
    if op == 1:
        return torch.where(d(b) > 0, a64, torch.zeros_like(a64))
    if op == 2:
        return 1.0 / (1.0 + torch.exp(-a64))
    if op == 3:
        return a64 * d(b) * (1.0 - d(b))
    if op == 4:
        return a64 + d(b)
    if op == 5:
        return a64 + d(b)[0]
    raise ValueError(op)


def elementwise_f32(op, a, b):
    """Ops 0, 4, 5 as the same single fp32 operations."""
    if op == 0:
        return torch.clamp_min(a + b, 0.0)
    if op == 4:
        return a + b
    if op == 5:
        return a + b[0]
    raise ValueError(op)


# ---------------------------------------------------------------------------------------------- row / column pieces on [M, C]
def rowscale(x, s):
    """out[m][c] = x[m][c] s[m]"""
    return d(x) * d(s)[:, None]


def rowscale_f32(x, s):
    return x * s[:, None]


def outer(s, w):
    """out[m][c] = s[m] w[c]"""
    return d(s)[:, None] * d(w)[None, :]


def outer_f32(s, w):
    return s[:, None] * w[None, :]


def rowdot(a, b):
    """out[m] = sum_c a[m][c] b[m][c]; b may be a [C] vector.  Returns (sum, sum of |terms|)."""
    t = d(a) * (d(b) if b.dim() == 2 else d(b)[None, :])
    return t.sum(1), t.abs().sum(1)


def rowscale_backward(dy, x, s):
    """The backward of out = x s[m]: dx = dy s[m], ds[m] = sum_c dy x.  Returns (dx, ds, sum_c |dy x|)."""
    t = d(dy) * d(x)
    return d(dy) * d(s)[:, None], t.sum(1), t.abs().sum(1)


def colsum(x, rows=None):
    """out[c] = sum_m rows[m] x[m][c] (rows = None: ones).  Returns (sum, sum of |terms|)."""
    t = d(x) if rows is None else d(x) * d(rows)[:, None]
    return t.sum(0), t.abs().sum(0)


def sum_n(srcs):
    """out = sum_k src_k.  Returns (sum, sum of |terms|)."""
    out, mag = d(srcs[0]).clone(), d(srcs[0]).abs()
    for s in srcs[1:]:
        out += d(s)
        mag += d(s).abs()
    return out, mag


def sum_n_f32(srcs):
    """fp32, left to right"""
    out = srcs[0].clone()
    for s in srcs[1:]:
        out = out + s
    return out


def slice_channels(x, c0, cs):
    return x[:, c0:c0 + cs].clone()


def pad_channels(x, cout):
    out = torch.zeros(x.shape[0], cout, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


# ---------------------------------------------------------------------------------------------- 2x2 windows on [B, H, W, C]
def _windows(t):
    """[B, H, W, C] -> the four [B, H/2, W/2, C] planes of the 2x2 windows in scan order (0,0), (0,1), (1,0), (1,1)."""
    return t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]


def sum2x2(dy):
    """The backward of a nearest x2 upsample: out[b][y][x][c] = the sum of dy's 2x2 block.  Returns (sum, sum of |terms|)."""
    w = [d(v) for v in _windows(dy)]
    return w[0] + w[1] + w[2] + w[3], w[0].abs() + w[1].abs() + w[2].abs() + w[3].abs()


def sum2x2_f32(dy):
    """fp32 as (a + b) + (c + d)"""
    a, b, c, e = _windows(dy)
    return (a + b) + (c + e)


def maxpool2_backward(x, dy):
    """MaxPool2d(2, 2) backward: dy goes to the window's FIRST maximum in scan order; a NaN takes over from whatever came before
    it (ATen's `val > max || isnan(val)`), so among several NaNs the LAST one receives dy.  Every other element of dx is 0.
    x [B, H, W, C], dy [B, H/2, W/2, C] -> dx like x (dy's dtype)."""
    v = _windows(x)
    best, arg = v[0].clone(), torch.zeros(v[0].shape, dtype=torch.long)
    for k in range(1, 4):
        take = (v[k] > best) | torch.isnan(v[k])
        best = torch.where(take, v[k], best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    dx = torch.zeros(x.shape, dtype=dy.dtype)
    for k, plane in enumerate(_windows(dx)):
        plane.copy_(torch.where(arg == k, dy, torch.zeros_like(dy)))
    return dx


# ---------------------------------------------------------------------------------------------- sparse value targets
def coords_in_range(coords, shape):
    """(channel, row, col) inside the map; the batch index is the caller's to keep inside [0, B) (only its sign is looked at)."""
    _, C, H, W = shape
    b, c, x, y = coords.unbind(1)
    return (b >= 0) & (c >= 0) & (c < C) & (x >= 0) & (x < H) & (y >= 0) & (y < W)


def gather_values(out1, coords):
    """pred[k] = out1[b, c, x, y], 0 for a coordinate outside the map.  out1 [B, C, H, W], coords int64 [K, 4]."""
    ok = coords_in_range(coords, out1.shape)
    pred = torch.zeros(coords.shape[0], dtype=out1.dtype)
    q = coords[ok]
    pred[ok] = out1[q[:, 0], q[:, 1], q[:, 2], q[:, 3]]
    return pred


def scatter_values(dpred, coords, shape):
    """d_out1[b, c, x, y] += dpred[k] (duplicates accumulate; coordinates outside the map add nothing).
    Returns (sum, sum of |terms|, multiplicity) per cell."""
    ok = coords_in_range(coords, shape)
    q = coords[ok]
    idx = (q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    v = d(dpred)[ok]
    out = torch.zeros(shape, dtype=torch.float64).index_put_(idx, v, accumulate=True)
    mag = torch.zeros(shape, dtype=torch.float64).index_put_(idx, v.abs(), accumulate=True)
    mult = torch.zeros(shape, dtype=torch.float64).index_put_(idx, torch.ones_like(v), accumulate=True)
    return out, mag, mult


# ---------------------------------------------------------------------------------------------- losses
def loss_terms(mode, p, t):
    """Per-element loss.  mode 0: (p - t)^2.  mode 1: -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)), where 1 - p is
    formed in fp32 as the kernel forms it (for p below 2^-25 that is 1, and the term is 0, not p)."""
    if mode == 0:
        return (d(p) - d(t)) ** 2
    q = d(1.0 - p)                                                   # fp32 subtraction
    lp = torch.clamp_min(torch.log(d(p)), LOG_CLAMP)
    lq = torch.clamp_min(torch.log(q), LOG_CLAMP)
    return -(d(t) * lp + (1.0 - d(t)) * lq)


def loss_sum(mode, p, t):
    """Returns (sum of the terms, sum of |terms|)."""
    terms = loss_terms(mode, p, t)
    return terms.sum(), terms.abs().sum()


def loss_grad(mode, p, t, coef=1.0):
    """coef d(mean loss)/dp.  mode 0: 2 (p - t) coef / n.  mode 1: (p - t) / max(p (1 - p), 1e-12) coef / n (1 - p in fp32)."""
    n = p.numel()
    c = float(torch.tensor(coef, dtype=torch.float32))               # the entry point takes a float
    if mode == 0:
        return 2.0 * (d(p) - d(t)) * c / n
    den = torch.clamp_min(d(p) * d(1.0 - p), GRAD_CLAMP)
    return (d(p) - d(t)) / den * c / n


# ---------------------------------------------------------------------------------------------- BatchNorm, the gate's middle
def _bn_rows(v, gamma, beta, eps):
    """F.batch_norm in training mode over the rows of v [M, C]"""
    return F.batch_norm(v.t().unsqueeze(0), None, None, gamma, beta, True, 0.0, eps).squeeze(0).t()


def batch_norm_train(x, gamma, beta, relu, dy, eps=1e-5):
    """Float64 autograd of F.batch_norm in training mode over the rows of x [M, C] (+ ReLU) on the fp32 inputs.
    Returns y, (dx, dgamma, dbeta) for dy, the batch mean and the UNBIASED batch variance (what the running statistics take)."""
    x64, g, b = [d(t).clone().requires_grad_(True) for t in (x, gamma, beta)]
    y = _bn_rows(x64, g, b, eps)
    if relu:
        y = torch.relu(y)
    y.backward(d(dy))
    return y.detach(), (x64.grad, g.grad, b.grad), d(x).mean(0), d(x).var(0, unbiased=True)


def gate_preactivation(gp, xp, gam_g, bet_g, gam_x, bet_x, eps=1e-5):
    """BN_g(g_pre) + BN_x(x_pre) in float64: what the gate's ReLU sees (a test keeps its gradient away from the rows where this
    is too close to zero for fp32 to call the sign)."""
    with torch.no_grad():
        return _bn_rows(d(gp), d(gam_g), d(bet_g), eps) + _bn_rows(d(xp), d(gam_x), d(bet_x), eps)


def gate_middle(gp, xp, gam_g, bet_g, gam_x, bet_x, w, b, dp, eps=1e-5):
    """The attention gate between its 1x1 convolutions and the sigmoid, unfused, in float64 autograd:
    p = relu(BN_g(g_pre) + BN_x(x_pre)) . w + b (train-mode BatchNorms over the rows of [M, F]).
    Returns p [M] and the gradients of (g_pre, x_pre, gamma_g, beta_g, gamma_x, beta_x, w, b) for dp."""
    leaves = [d(t).clone().requires_grad_(True) for t in (gp, xp, gam_g, bet_g, gam_x, bet_x, w, b)]
    g0, x0, gg, bg, gx, bx, w0, b0 = leaves
    q = torch.relu(_bn_rows(g0, gg, bg, eps) + _bn_rows(x0, gx, bx, eps))
    p = (q * w0[None, :]).sum(1) + b0[0]
    p.backward(d(dp))
    return p.detach(), [t.grad for t in leaves]
