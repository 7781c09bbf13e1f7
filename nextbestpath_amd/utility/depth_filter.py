"""The depth-frame filter: the DEFINITION (numpy, CPU) that csrc/nbp_depth_filter.hip equals bit for bit.
Not in the reference, which consumes its depth maps as they come.

One pass over a raw frame z [H,W] fp32 (z = -1: no return); every decision reads the raw frame only, and every output value is an
element of the input or -1.  Terms:
    valid(q)  <=>  z_q > -1                                            (NaN is invalid)
    N(p)      =    the pixels q != p with Chebyshev distance <= radius that lie inside the image
    gate(c)   :    t = c c;  t = range_quad t;  t = range_base + t      (fp32, in this order, no contraction)
Valid centre z:   S = {z_q : q in N(p), valid(q), |z_q - z| <= gate(z)} (fp32 subtract, abs, <=), n = |S|.
    n < min_support      -> -1                                          (speckle and flying-pixel rejection)
    else, smooth         -> the element of rank n // 2 (0-based, ascending) of S + {z}: the median, the lower one when n + 1 is even
    else                 -> z
Invalid centre:   V = {z_q : q in N(p), valid(q)}.
    fill_support == 0 or |V| < fill_support -> -1
    else m = the element of rank (|V| - 1) // 2 of V;  m when every v in V has |v - m| <= gate(m), else -1 (no fill across an edge)
On a straight silhouette a background pixel has 3 of its 8 neighbours invalid at radius 1, 10 of 24 at radius 2: fill_support >= 6
(radius 1) or >= 18 (radius 2) does not dilate objects.

Selection is by value, by counting: the answer is the smallest candidate c of the window for which at least rank + 1 members are
<= c.  The window is symmetric, so the definition is EXACTLY equivariant under the eight symmetries of the image (flips, transpose,
quarter turns): apply(op(z)) == op(apply(z)) bit for bit.  (The one freedom by-value selection leaves is a window that holds both
-0 and +0, which compare equal: there the first candidate in row-major window order wins, here and in the kernel.  Depths of a
camera are positive.)
"""
from __future__ import annotations

import math
import numbers

import numpy as np

f32 = np.float32

MAX_PIXELS = 1 << 29

_KEYS = ("radius", "range_base", "range_quad", "smooth", "min_support", "fill_support")


def option_spec(x):
    """The option `depth_filter` -> None (off) or the normalised spec: a dict with exactly the keys radius (1 or 2: a 3 x 3 or 5 x 5
    window; default 1), range_base, range_quad (floats, finite and >= 0, at least one > 0; a missing one is 0, and the pair has no
    default and no `True` preset: they are meant as a multiple of the noise model's sigma_base / sigma_quad, and nobody has measured a
    sensor in these scene units), smooth (bool; default True), min_support (int in 0 .. (2 radius + 1)^2 - 1; default 0 = off) and
    fill_support (int, 0 = off or 1 .. (2 radius + 1)^2 - 1; default 0).  None = off.  ValueError on anything else: another type,
    unknown keys, bools where numbers are expected (and numbers where the bool is), values out of range, both ranges 0."""
    if x is None:
        return None
    if not isinstance(x, dict):
        raise ValueError("depth_filter: None or a dict with the keys " + " / ".join(_KEYS) + " expected")
    unknown = sorted(set(x) - set(_KEYS), key=str)
    if unknown:
        raise ValueError(f"depth_filter: unknown keys {unknown}")
    out = {}
    r = x.get("radius", 1)
    if isinstance(r, bool) or not isinstance(r, numbers.Integral) or r not in (1, 2):
        raise ValueError(f"depth_filter: radius must be 1 or 2, got {r!r}")
    out["radius"] = int(r)
    for k in ("range_base", "range_quad"):
        v = x.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
            raise ValueError(f"depth_filter: {k} must be a finite non-negative number, got {v!r}")
        out[k] = float(v)
    if not (f32(out["range_base"]) > 0 or f32(out["range_quad"]) > 0):
        raise ValueError("depth_filter: range_base or range_quad must be positive (there is no default gate)")
    s = x.get("smooth", True)
    if not isinstance(s, (bool, np.bool_)):
        raise ValueError(f"depth_filter: smooth must be a bool, got {s!r}")
    out["smooth"] = bool(s)
    top = (2 * out["radius"] + 1) ** 2 - 1
    for k in ("min_support", "fill_support"):
        v = x.get(k, 0)
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= top:
            raise ValueError(f"depth_filter: {k} must be an integer in 0 .. {top} at radius {out['radius']}, got {v!r}")
        out[k] = int(v)
    return out


def gate(c, spec):
    """gate(c) on an fp32 array: three fp32 operations, each rounded on its own."""
    t = c * c
    t = f32(spec["range_quad"]) * t
    return f32(spec["range_base"]) + t


def apply(z_raw, spec):
    """z_raw [H,W] fp32, spec (option_spec's or its argument) -> the filtered frame [H,W] fp32."""
    spec = option_spec(spec)
    if spec is None:
        raise ValueError("depth_filter.apply needs a spec (None means off: there is nothing to apply)")
    z = np.ascontiguousarray(z_raw, f32)
    if z.ndim != 2 or z.size < 1 or z.size > MAX_PIXELS:
        raise ValueError(f"depth_filter.apply: one [H,W] frame of at most 2^29 pixels expected, got shape {z.shape}")
    H, W = z.shape
    r = spec["radius"]
    D = 2 * r + 1
    K, C = D * D, r * D + r
    none, nan = f32(-1.0), f32(np.nan)
    pad = np.full((H + 2 * r, W + 2 * r), none, f32)               # outside the image: -1, which is "invalid"
    pad[r:r + H, r:r + W] = z
    win = [pad[k // D:k // D + H, k % D:k % D + W] for k in range(K)]      # row-major window order; win[C] is z
    centre = z > none
    with np.errstate(all="ignore"):
        tau = gate(z, spec)
        # the members of the selection: NaN where a pixel takes no part (NaN <= c is false: it never counts, and is never chosen)
        w, n = [None] * K, np.zeros((H, W), np.int32)
        for k in range(K):
            if k == C:
                continue
            v = win[k]
            ok = v > none
            member = np.where(centre, ok & (np.abs(v - z) <= tau), ok)
            n += member
            w[k] = np.where(member, v, nan)
        w[C] = np.where(centre, z, nan)
        need = np.where(centre, n // 2, (n - 1) // 2) + 1          # rank + 1
        best = np.full((H, W), f32(np.inf), f32)
        for i in range(K):
            c = w[i]
            cnt = np.zeros((H, W), np.int32)
            for k in range(K):
                cnt += w[k] <= c
            best = np.where((cnt >= need) & (c < best), c, best)
        edge = np.zeros((H, W), bool)                              # invalid centre: a valid neighbour outside the gate of m = best
        tau_m = gate(best, spec)
        for k in range(K):
            if k != C:
                edge |= (w[k] > none) & ~(np.abs(w[k] - best) <= tau_m)
    kept = np.where(n < spec["min_support"], none, best if spec["smooth"] else z)
    fill = spec["fill_support"]
    filled = np.where((n >= max(fill, 1)) & ~edge, best, none) if fill > 0 else np.full((H, W), none, f32)
    return np.where(centre, kept, filled).astype(f32)
