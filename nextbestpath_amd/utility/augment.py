"""The eight symmetries of the square (D4) acting on an NBP training record: host side, numpy, small.

The reference defines ``augment_data`` (next_best_path/utility/nbp_utils.py:267-289: flips and 90-degree rotations, p = 0.4) and
never calls it.  As written it could not be used: it turns only the images, the sparse targets ``(heading, row, col)`` stay where
they were, and an array flip ``i -> S-1-i`` moves the input by one pixel (0.31 units) but the value map by one cell (1.25 units).

Everything here is the GEOMETRIC action about the camera, NOT an array flip.  The maps are a translation-only window around the
camera and pixel index ``i = rint((v + 40) n / 80)`` puts the camera at ``n / 2`` on a grid of side ``n`` (the input grid ``S`` and
the value grid ``V = S / 4`` alike), so the reflection ``v -> -v`` is ``i -> n - i``: index 0 (the half-width bin at the window's far
edge) has its mirror image, index ``n``, outside the array, and comes out zero.

An element is an op code 0..7: bit 0 = transpose (rows <-> cols), bit 1 = reflect rows, bit 2 = reflect cols, applied in that order.

    transpose       out[r][c] = in[c][r]
    reflect rows    out[r][c] = in[n - r][c] for r >= 1, out[0][c] = 0          (reflect cols likewise)

Heading channel ``h`` looks along ``(x, z) = (sin a, cos a)``, ``a = 45 h`` degrees (simulator/camera.py); the image axes are
``row ~ -(z - c_z)``, ``col ~ -(x - c_x)``, so it points along ``(d_row, d_col) = (-cos a, -sin a)`` and the three generators
permute the channels: transpose ``h -> (2 - h) mod 8``, reflect rows ``h -> (4 - h) mod 8``, reflect cols ``h -> -h mod 8``
(tests/test_augment_host.py derives them again from the camera code).

The images of a batch are moved on the device by ``hipops.augment_batch`` (nbp_augment_batch_f32); ``transform_maps`` is the same
action in numpy for tests and small arrays.
"""
from __future__ import annotations

import numpy as np

N_OPS = 8
TRANSPOSE, REFLECT_ROWS, REFLECT_COLS = 1, 2, 4


def _check(op):
    op = int(op)
    if not 0 <= op < N_OPS:
        raise ValueError(f"augment op code {op} outside 0..7")
    return op


def heading_map(op):
    """int64[8]: the heading channel that channel h of a value map becomes under `op`."""
    op = _check(op)
    h = np.arange(8, dtype=np.int64)
    if op & TRANSPOSE:
        h = (2 - h) % 8
    if op & REFLECT_ROWS:
        h = (4 - h) % 8
    if op & REFLECT_COLS:
        h = (-h) % 8
    return h


def transform_maps(a, op):
    """`op` on the last two (square) axes of `a`: a new array, the reflection about the camera with its zero row / column."""
    op = _check(op)
    a = np.asarray(a)
    if a.shape[-1] != a.shape[-2]:
        raise ValueError("transform_maps: square planes expected")
    out = np.swapaxes(a, -1, -2) if op & TRANSPOSE else a
    if op & REFLECT_ROWS:
        r = np.zeros_like(out)
        r[..., 1:, :] = out[..., :0:-1, :]
        out = r
    if op & REFLECT_COLS:
        r = np.zeros_like(out)
        r[..., :, 1:] = out[..., :, :0:-1]
        out = r
    return np.array(out, copy=True, order="C")


def transform_targets(pixels, gains, op, V):
    """(heading, row, col) int64 [K,3] and their gains [K] under `op` on a V x V value grid -> (pixels', gains'), new arrays.
    A target whose cell leaves the grid (a coordinate 0 that is reflected) is DROPPED together with its gain."""
    op = _check(op)
    px = np.array(pixels, dtype=np.int64, copy=True).reshape(-1, 3)
    g = np.array(gains, copy=True).reshape(-1)
    if len(px) != len(g):
        raise ValueError("transform_targets: one gain per target expected")
    if op == 0:
        return px, g
    h, r, c = heading_map(op)[px[:, 0]], px[:, 1], px[:, 2]
    if op & TRANSPOSE:
        r, c = c, r
    keep = np.ones(len(px), dtype=bool)
    if op & REFLECT_ROWS:
        keep &= r >= 1
        r = V - r
    if op & REFLECT_COLS:
        keep &= c >= 1
        c = V - c
    return np.stack([h, r, c], 1)[keep], g[keep]


def draw_ops(rng, n, p):
    """int32[n]: per sample, with probability `p` one of the seven non-identity elements, uniformly, else 0.  `rng` is a
    random.Random of the caller's (never the global generator); nothing is drawn from it when p <= 0."""
    ops = np.zeros(int(n), dtype=np.int32)
    if p <= 0:
        return ops
    for i in range(len(ops)):
        if rng.random() < p:
            ops[i] = 1 + rng.randrange(N_OPS - 1)
    return ops


def augment_records(records, ops, V):
    """Shallow copies of replay records with their targets moved by ops[i] (the images are moved on the device after collation);
    identity samples are passed through as they are.  The records themselves are never modified."""
    out = []
    for d, op in zip(records, ops):
        if int(op):
            d = dict(d)
            d["target_value_map_pixel"], d["actual_coverage_gain"] = transform_targets(
                d["target_value_map_pixel"], d["actual_coverage_gain"], int(op), V)
        out.append(d)
    return out
