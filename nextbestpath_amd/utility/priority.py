"""Loss-prioritised replay: the numpy definitions of record (host).  csrc/nbp_objective.hip computes the per-sample terms of the
training objective on the device (hipops.objective_forward / objective_backward, networks/training.py::ObjectiveFn);
tests/test_gpu_objective.py holds the kernels to `objective_reference`.  Not in the reference, whose trainer visits every record of
the replay list once per inner epoch (nbp_utils.py:340-395); off unless the trainer's `replay_priority_alpha` is set.

Per sample b of a batch (out1 [B,C,H,W], coords_bcxy [K,4] = (b, c, x, y) in any row order, gains [K], out2 / gt [B,S,S]):

  v_b = sum over the rows k with b_k = b of (out1[b,c,x,y] - gain_k)^2       n_b = the number of those rows
  o_b = sum over the pixels of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))

A row with a coordinate out of range contributes nothing (neither to v nor to n).  With per-sample weights w (1 when None):

  mse = sum_b w_b v_b / K        bce = sum_b w_b o_b / (B S^2)          (the UNWEIGHTED denominators; K = 0: mse = 0)

so that w = 1 gives F.mse_loss / F.binary_cross_entropy as the trainer has them.  Gradients of coef0 mse + coef1 bce:

  d_out1[b,c,x,y] += coef0 w_b 2 (pred - gain) / K   (repeated cells add)
  d_out2           = coef1 w_b (p - t) / max(p (1 - p), 1e-12) / (B S^2)       (the expression of loss_grad_kernel)

The priority of a sample is its own share of NBP.loss without the additive log-variance terms (`sample_loss`).

Proportional prioritisation after Schaul et al., "Prioritized Experience Replay", ICLR 2016: record i with last loss
l_i is drawn with probability P_i = q_i / sum q, q_i = (l_i + eps)^alpha, and its term of the objective is weighted with
w_i = (N P_i)^-beta / max_j (N P_j)^-beta <= 1, which undoes (beta = 1: fully) the bias of the non-uniform draw."""
from __future__ import annotations

import math

import numpy as np


def objective_reference(out1, coords_bcxy, gains, out2, gt, weights=None, coef=(1, 1)):
    """The objective of one batch in float64 from the fp32 (or any) inputs -> dict: per_sample [B,3] (v_b, n_b, o_b), totals [2]
    (sum w v, sum w o), mse, bce, d_out1 [B,C,H,W], d_out2 (the shape of out2)."""
    out1 = np.asarray(out1, dtype=np.float64)
    p = np.asarray(out2, dtype=np.float64)
    t = np.asarray(gt, dtype=np.float64)
    coords = np.asarray(coords_bcxy, dtype=np.int64).reshape(-1, 4)
    gains = np.asarray(gains, dtype=np.float64).reshape(-1)
    B, C, H, W = out1.shape
    K = coords.shape[0]
    if gains.shape[0] != K or p.shape[0] != B or t.shape != p.shape:
        raise ValueError("objective_reference: out1 [B,C,H,W], coords [K,4], gains [K], out2 / gt [B,...] expected")
    w = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64).reshape(B)
    n_px = int(np.prod(p.shape[1:]))
    per_sample = np.zeros((B, 3))
    d_out1 = np.zeros_like(out1)
    ok = ((coords >= 0) & (coords < np.array([B, C, H, W]))).all(1) if K else np.zeros(0, bool)
    for k in np.nonzero(ok)[0]:
        b, c, x, y = coords[k]
        d = out1[b, c, x, y] - gains[k]
        per_sample[b, 0] += d * d
        per_sample[b, 1] += 1
        d_out1[b, c, x, y] += coef[0] * w[b] * 2.0 * d / K
    with np.errstate(divide="ignore"):
        terms = -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - p), -100.0))
    per_sample[:, 2] = terms.reshape(B, -1).sum(1)
    totals = np.array([(w * per_sample[:, 0]).sum(), (w * per_sample[:, 2]).sum()])
    wb = w.reshape((B,) + (1,) * (p.ndim - 1))
    d_out2 = coef[1] * wb * (p - t) / np.maximum(p * (1.0 - p), 1e-12) / (B * n_px)
    return {"per_sample": per_sample, "totals": totals, "mse": totals[0] / K if K else 0.0, "bce": totals[1] / (B * n_px),
            "d_out1": d_out1, "d_out2": d_out2}


def sample_loss(per_sample, S, log_vars):
    """l_b = v_b / max(n_b, 1) / (2 e^{2 s0}) + (o_b / S^2) / e^{2 s1}: the sample's own share of NBP.loss without the additive s
    terms.  per_sample [B,3] (v, n, o), log_vars (s0, s1) -> float64 [B]."""
    ps = np.asarray(per_sample, dtype=np.float64).reshape(-1, 3)
    s0, s1 = float(log_vars[0]), float(log_vars[1])
    return ps[:, 0] / np.maximum(ps[:, 1], 1.0) / (2.0 * math.exp(2.0 * s0)) + (ps[:, 2] / (float(S) * float(S))) / math.exp(2.0 * s1)


def check_options(alpha, beta=0.4, eps=1e-3, seed=None):
    """The trainer's replay_priority_* options -> None (alpha None: off) or a dict of checked values; ValueError otherwise."""
    def number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    if alpha is None:
        return None
    if not number(alpha) or alpha < 0:
        raise ValueError(f"replay_priority_alpha must be null or a number >= 0, not {alpha!r}")
    if not number(beta) or not 0 <= beta <= 1:
        raise ValueError(f"replay_priority_beta must be a number in [0, 1], not {beta!r}")
    if not number(eps) or not eps > 0:
        raise ValueError(f"replay_priority_eps must be a number > 0, not {eps!r}")
    if seed is not None and (not isinstance(seed, int) or isinstance(seed, bool) or seed < 0):
        raise ValueError(f"replay_priority_seed must be null or an integer >= 0, not {seed!r}")
    return {"alpha": float(alpha), "beta": float(beta), "eps": float(eps), "seed": seed}


class ReplayPriorities:
    """The table record key -> last sample loss l, and the draws from it.  A record never trained on has the largest l seen so far
    (1.0 before any has been seen), so that it is drawn soon.  `begin(keys)` names the population of an inner epoch; `draw` then
    returns positions in that list with their weights, from the table as it stands at the time of the call."""

    def __init__(self, alpha=0.6, beta=0.4, eps=1e-3):
        opts = check_options(alpha, beta, eps)
        if opts is None:
            raise ValueError("ReplayPriorities needs an alpha (None switches the feature off in the trainer)")
        self.alpha, self.beta, self.eps = opts["alpha"], opts["beta"], opts["eps"]
        self.table = {}
        self.max_seen = None
        self.keys = []
        self.counts = np.zeros(0, np.int64)
        self.min_weight = None

    def initial(self):
        """l of a record that has never been trained on."""
        return 1.0 if self.max_seen is None else self.max_seen

    def losses(self, keys):
        init = self.initial()
        return np.array([self.table.get(k, init) for k in keys], dtype=np.float64)

    def probabilities(self, keys, alpha=None, eps=None):
        """P_i = q_i / sum q with q_i = (l_i + eps)^alpha over `keys` (float64)."""
        q = self._q(keys, alpha, eps)
        return q / q.sum()

    def _q(self, keys, alpha=None, eps=None):
        alpha = self.alpha if alpha is None else alpha
        eps = self.eps if eps is None else eps
        return np.power(self.losses(keys) + eps, alpha)

    def weights(self, keys, beta=None):
        """w_i = (N P_i)^-beta / max_j (N P_j)^-beta over `keys`: at most 1, and 1 for the least likely record."""
        beta = self.beta if beta is None else beta
        P = self.probabilities(keys)
        w = np.power(len(keys) * P, -beta)
        return w / w.max()

    def begin(self, keys):
        """The population of the draws that follow; the draw statistics start again."""
        self.keys = list(keys)
        self.counts = np.zeros(len(self.keys), np.int64)
        self.min_weight = None

    def draw(self, rng, n):
        """n positions in the population, with replacement, and their weights (float64): u ~ U[0,1) from the seeded
        np.random.Generator `rng`, the position by searchsorted in the cumulative sum of P."""
        N = len(self.keys)
        if N < 1:
            raise ValueError("ReplayPriorities.draw: empty population (call begin(keys) first)")
        P = self.probabilities(self.keys)
        cum = np.cumsum(P)
        idx = np.minimum(np.searchsorted(cum, rng.random(int(n)) * cum[-1], side="right"), N - 1)
        w = np.power(N * P, -self.beta)
        w = w / w.max()
        np.add.at(self.counts, idx, 1)
        if len(idx):
            m = float(w[idx].min())
            self.min_weight = m if self.min_weight is None else min(self.min_weight, m)
        return idx, w[idx]

    def update(self, keys, losses):
        """Stores the new l of the records `keys` (a key named twice keeps the last)."""
        for k, v in zip(keys, np.asarray(losses, dtype=np.float64).reshape(-1)):
            v = float(v)
            self.table[k] = v
            if math.isfinite(v) and (self.max_seen is None or v > self.max_seen):
                self.max_seen = v

    def stats(self):
        """Over the current population: the effective sample size (sum q)^2 / (N sum q^2) (1 = uniform), min / mean / max l, the
        smallest weight handed out and the fraction of distinct records drawn since begin()."""
        N = len(self.keys)
        if N < 1:
            return {"n": 0}
        q = self._q(self.keys)
        l = self.losses(self.keys)
        return {"n": N, "effective_sample_size": float(q.sum() ** 2 / (N * (q * q).sum())), "loss_min": float(l.min()),
                "loss_mean": float(l.mean()), "loss_max": float(l.max()),
                "min_weight": None if self.min_weight is None else float(self.min_weight),
                "draws": int(self.counts.sum()), "distinct_fraction": float((self.counts > 0).sum() / N)}
