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

The same action serves inference: the SYMMETRY ENSEMBLE of the eval forward (``NBP.symmetry_ensemble``) runs the network on the
moved copies ``g_k x`` of its input, moves every output back with ``g_k^-1`` and averages.  ``ENSEMBLES`` names the subsets,
``ensemble_reference`` is the definition in float64; the device side is ``hipops.symmetry_expand`` / ``symmetry_reduce``
(csrc/nbp_ensemble.hip).
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


def inverse_op(op):
    """Op code of the inverse element.  With the code order transpose, reflect rows, reflect cols the two quarter turns 3 and 5 are
    each other's inverse and every other element is its own (tests/test_ensemble_host.py finds them again by brute force)."""
    op = _check(op)
    return {3: 5, 5: 3}.get(op, op)


def transform_value_map(y, op):
    """`op` on a value map [..., 8, V, V]: the planes move as in transform_maps and channel heading_map(op)[h] of the result is the
    moved plane h -- dense content moves exactly as transform_targets moves the sparse targets."""
    op = _check(op)
    y = np.asarray(y)
    if y.ndim < 3 or y.shape[-3] != 8:
        raise ValueError("transform_value_map: [..., 8, V, V] expected")
    out = np.empty_like(transform_maps(y, op))
    out[..., heading_map(op), :, :] = transform_maps(y, op)
    return out


# the named symmetry ensembles: subsets of D4 that hold the identity (first) and the inverse of each of their elements
ENSEMBLES = {"c2": (0, 6), "flips": (0, 2, 4, 6), "d4": tuple(range(N_OPS))}


def check_ensemble(spec):
    """None, a name of ENSEMBLES, or a sequence of distinct op codes that starts with 0 -> None or the tuple of op codes."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in ENSEMBLES:
            raise ValueError(f"unknown symmetry ensemble {spec!r} (known: {sorted(ENSEMBLES)})")
        return ENSEMBLES[spec]
    try:
        ops = tuple(spec)
    except TypeError:
        raise ValueError(f"symmetry ensemble: None, a name or a sequence of op codes expected, got {spec!r}") from None
    for op in ops:
        if isinstance(op, (bool, str, float)) or not isinstance(op, (int, np.integer)) or not 0 <= int(op) < N_OPS:
            raise ValueError(f"symmetry ensemble: op code {op!r} outside 0..7")
    ops = tuple(int(op) for op in ops)
    if not ops or ops[0] != 0:
        raise ValueError("symmetry ensemble: the first member must be the identity (op code 0)")
    if len(set(ops)) != len(ops):
        raise ValueError(f"symmetry ensemble: duplicate op codes in {ops}")
    return ops


def ensemble_reference(raw1, raw2, ops):
    """The symmetry ensemble, in float64.  raw1 [n,B,8,V,V] and raw2 [n,B,1,S,S] are the network's outputs on the moved inputs,
    raw[k] = f(g_k x) with g_k = ops[k].  Plane k is moved back by inverse_op(ops[k]) (transform_value_map / transform_maps), the
    planes are summed and every cell is divided by the number of members that reach it: a member whose inverse reflects rows says
    nothing about row 0, whose mirror image lies outside the window (likewise columns), so that the ensemble of a constant,
    heading-independent map is that constant everywhere, edge included.  The identity reaches every cell.  -> (out1, out2)."""
    ops = check_ensemble(ops)
    raw1, raw2 = np.asarray(raw1, np.float64), np.asarray(raw2, np.float64)
    if ops is None or raw1.ndim != 5 or raw2.ndim != 5 or raw1.shape[0] != len(ops) or raw2.shape[0] != len(ops):
        raise ValueError("ensemble_reference: raw1 [n,B,8,V,V], raw2 [n,B,1,S,S] and n op codes expected")
    outs = []
    for raw, move in ((raw1, transform_value_map), (raw2, transform_maps)):
        side = raw.shape[-1]
        total, count = np.zeros(raw.shape[1:]), np.zeros((side, side))
        for k, op in enumerate(ops):
            g = inverse_op(op)
            total += move(raw[k], g)
            reach = np.ones((side, side))
            if g & REFLECT_ROWS:
                reach[0, :] = 0
            if g & REFLECT_COLS:
                reach[:, 0] = 0
            count += reach
        outs.append(total / count)
    return outs[0], outs[1]


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
