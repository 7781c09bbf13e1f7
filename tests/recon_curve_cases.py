"""The chunk sequence that the per-step reconstruction curve's host and GPU tests share (tests/test_recon_curve_host.py,
tests/test_gpu_recon_curve.py), and its whole-cloud references, computed once per process."""
import functools

import numpy as np

from nextbestpath_amd.utility import recon_metrics as rm

f32 = np.float32
THRESHOLDS, CAP = (0.5, 1.0, 2.0), 5.0
# 0: an update with nothing new (first, and in the middle); 7 / 8 / 9: around the 8 lanes of a point; 255 / 256 / 257: around a
# block's 256 threads; 12000 points: several passes of a grid sized by a smaller host bound
SIZES = [0, 1, 7, 8, 9, 255, 256, 257, 0, 3000, 12000]
PREFIXES = (1, 4, 7, 9, 10)               # whole-cloud references after these chunks (0-based, inclusive)


@functools.lru_cache(maxsize=None)
def plane_case():
    """-> (gt [3000,3] with one duplicated point, chunks).  The chunks march over two thirds of the plane (x up to 20 of 30), so that
    the recall never saturates; 15 % of every chunk are uniform outliers that reach beyond the grown box; one point equals a GT
    point."""
    rng = np.random.default_rng(77)
    gt = np.stack([rng.uniform(0, 30, 3000), np.full(3000, 2.0), rng.uniform(0, 20, 3000)], 1).astype(f32)
    gt[1] = gt[0]
    chunks = []
    for k, n in enumerate(SIZES):
        x0, x1 = 20.0 * k / len(SIZES), 20.0 * (k + 1) / len(SIZES)
        near = np.stack([rng.uniform(x0, x1, n), 2.0 + rng.normal(0, 0.4, n), rng.uniform(-1, 21, n)], 1)
        outl = rng.uniform([-8, -8, -8], [38, 12, 28], (n, 3))
        c = np.where((rng.uniform(size=n) < 0.15)[:, None], outl, near).astype(f32)
        if n == 257:
            c[100] = gt[2000]                                      # a new point exactly on a GT point
        chunks.append(c)
    for c in chunks:
        c.setflags(write=False)
    gt.setflags(write=False)
    return gt, tuple(chunks)


@functools.lru_cache(maxsize=None)
def plane_states():
    """The incremental definition run over the chunks -> [(row, d2_gt, acc_sums, acc_counts, n_rec)] after every update."""
    gt, chunks = plane_case()
    ref = rm.CurveReference(gt, THRESHOLDS, CAP)
    out = []
    for c in chunks:
        row = ref.update(c)
        out.append((row.copy(), ref.d2_gt.copy(), ref.acc_sums.copy(), ref.acc_counts.copy(), ref.n_rec))
    return out


@functools.lru_cache(maxsize=None)
def plane_whole(k):
    """The whole-cloud definition over chunks 0..k -> (acc_sums, acc_counts, n, comp_sums, comp_counts, d2_gt)."""
    gt, chunks = plane_case()
    cloud = np.concatenate(chunks[:k + 1])
    lo, hi = rm.grown_box(gt.min(0), gt.max(0), CAP)
    acc = rm.stats_reference(rm.nn_dist2_reference(cloud, gt, lo, hi, CAP), THRESHOLDS)
    d2_gt = rm.nn_dist2_reference(gt, cloud, lo, hi, CAP)
    comp = rm.stats_reference(d2_gt, THRESHOLDS)
    return acc[0], acc[1], len(cloud), comp[0], comp[1], d2_gt
