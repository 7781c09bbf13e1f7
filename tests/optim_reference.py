"""Float64 numpy restatement of the optimizer step of nextbestpath_amd/optim.py (torch.optim.AdamW's rule behind
torch.nn.utils.clip_grad_norm_'s coefficient), and the rounding-error bounds the fp32 kernels are held to.

    coef = min(1, max_norm / (total_norm + 1e-6))            (1 without clipping)
    g^ = coef g;  p <- p (1 - lr wd);  m <- beta1 m + (1 - beta1) g^;  v <- beta2 v + (1 - beta2) g^^2
    p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),     bc1 = 1 - beta1^step, bc2 = 1 - beta2^step

tests/test_optim_host.py pins it to torch.optim.AdamW on CPU float64 tensors."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def total_norm(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)))


def clip_coef(grads, max_norm):
    """clip_grad_norm_'s coefficient in float64 (1.0 when max_norm is None)."""
    if max_norm is None:
        return 1.0
    return min(1.0, float(max_norm) / (total_norm(grads) + 1e-6))


def adamw_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, coef=1.0):
    """One step for one tensor; `step` is the counter AFTER the increment (1 for the first step).  Inputs of any float dtype are
    taken to float64.  -> dict with the new p, m, v and the terms the error bounds are written in."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    gh = coef * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    m2 = beta1 * m + (1.0 - beta1) * gh
    v2 = beta2 * v + (1.0 - beta2) * gh * gh
    denom = np.sqrt(v2) / np.sqrt(bc2) + eps
    p2 = p * (1.0 - lr * weight_decay) - (lr / bc1) * m2 / denom
    return {"p": p2, "m": m2, "v": v2, "denom": denom, "bc1": bc1, "gh": gh,
            "m_terms": beta1 * np.abs(m) + (1.0 - beta1) * np.abs(gh)}


def bounds(p, ref, lr, beta1=0.9, beta2=0.999, clipped=False):
    """The absolute error allowed on (m, v, p) for a kernel that rounds to fp32, from the count of roundings (u = 2^-24):
        |m' - m64| <= 4u (beta1 |m| + (1 - beta1) |g^|)
        |v' - v64| <= 6u v64
        |p' - p64| <= 3u |p| + 16u lr (beta1 |m| + (1 - beta1) |g^|) / (bc1 denom64)
    clipped: the coefficient is an fp32 number on the device and g^ = fl(coef g) one more rounding, so g^ carries a relative error of
    2u against coef64 g.  Each bound grows by 2u times the size of what g^ feeds into it: (1 - beta1) |g^| for m, twice
    (1 - beta2) g^^2 for v (the square doubles a relative error), and lr (1 - beta1) |g^| / (bc1 denom64) for p."""
    p = np.abs(np.asarray(p, dtype=np.float64))
    gh = np.abs(ref["gh"])
    upd = lr * ref["m_terms"] / (ref["bc1"] * ref["denom"])
    bm = 4 * U * ref["m_terms"]
    bv = 6 * U * ref["v"]
    bp = 3 * U * p + 16 * U * upd
    if clipped:
        bm = bm + 2 * U * (1.0 - beta1) * gh
        bv = bv + 2 * U * 2.0 * (1.0 - beta2) * gh * gh
        bp = bp + 2 * U * lr * (1.0 - beta1) * gh / (ref["bc1"] * ref["denom"])
    return bm, bv, bp
