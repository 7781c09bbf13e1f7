"""Frontier-based exploration (Yamauchi 1997) as a policy behind the network's interface: the DEFINITION (numpy, CPU) that
csrc/nbp_frontier.hip equals bit for bit.  Not in the reference.

The policy stands where the NBP network stands: from the six-channel map stack maps6 [6,S,S] of a step (S a multiple of 64,
V = S / 4) it computes the planner's two inputs, a value map out1 [8,V,V] and an obstacle map out2 [1,S,S].

Cell classes.  The domain D is the pixels with 1 <= row, col <= S - 1: row 0 and column 0 are the half-width bins whose mirror image
lies outside the window (utility/augment.py); they are never seen, never unknown, never frontier and never counted, which makes the
policy exactly D4-equivariant.
    seen(p)      p in D and any of maps6[0..4][p] > 0
    occupied(p)  p in D and maps6[5][p] > 0                 (the camera-height band: the planner's own obstacle evidence)
    free(p)      seen(p) and not occupied(p)
    near_d(p)    some q in D within Chebyshev distance d (`dilate`) of p is seen
    seen_d(p)    every q within Chebyshev distance d of p lies outside D or has near_d(q)
    unknown(p)   p in D and not seen_d(p)
    frontier(p)  free(p) and one of its four edge neighbours is unknown             (a neighbour outside D is not unknown)
seen_d is the morphological closing of `seen` by a (2 d + 1)-square: a dilation, which fills the pin-holes of the seen region (the
cloud is a 5 % sub-sample of the depth pixels), and an erosion, which takes the rim the dilation added away again, so that the
boundary of the seen region stays where it is and its free pixels still touch unknown space.  (The dilation alone would leave no
frontier for any d >= 1: every neighbour of a seen pixel is within distance 1 of it.)  seen implies seen_d; d = 0 is seen itself.

Sectors.  Heading channel h points along (d_row, d_col) = (-cos 45h deg, -sin 45h deg), DIRECTIONS[h] below without the 1 / sqrt 2
of the diagonals.  For an offset (dy, dx) let t be its component along the direction and s the absolute value of its component
across it (both without the common factor): the offset is in sector h iff t > 0 and (s + t)^2 < 2 t^2, i.e. |angle| < 22.5 deg.
Equality cannot occur in integers (sqrt 2 is irrational), so the eight sectors tile the punctured plane without ties.

Outputs.  Value cell g sits at pixel 4 g.  gain(h, g0, g1) = the number of frontier pixels (r, c) whose offset (dy, dx) =
(r - 4 g0, c - 4 g1) is non-zero, has dy^2 + dx^2 <= R^2 (`radius`) and lies in sector h.
    out1[h, g0, g1] = float(max(gain - distance_penalty * max(|g0 - V/2|, |g1 - V/2|), 0))
    out2[0, p]      = 1.0 where `unknown` == "obstacle" and unknown(p), else 0.0
Every count is an integer below 2^24: the floats are exact.

The defaults (radius 24, dilate 2, unknown "free", distance_penalty 0) are conventions, not measurements.
"""
from __future__ import annotations

import numbers

import numpy as np

NAME = "frontier"
MAX_RADIUS, MAX_DILATE = 31, 8
UNKNOWN_MODES = ("free", "obstacle")
# (d_row, d_col) of heading h, the diagonals without their 1 / sqrt 2
DIRECTIONS = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))

_DEFAULTS = {"radius": 24, "dilate": 2, "unknown": "free", "distance_penalty": 0}


def option_spec(x):
    """The planning option `policy` -> None (the network: nothing is built, launched or written) or the normalised spec: a dict
    with exactly the keys name ("frontier"), radius (1..31), dilate (0..8), unknown ("free" / "obstacle") and distance_penalty
    (an integer >= 0).  None and "nbp" = the network; "frontier" = the defaults; a dict {"name": "frontier", ...} with any of the
    other keys fills the rest with the defaults.  ValueError on anything else: another type or name, unknown keys, values out of
    range."""
    if x is None or x == "nbp":
        return None
    if isinstance(x, str):
        x = {"name": x}
    if not isinstance(x, dict):
        raise ValueError("policy: None, 'nbp', 'frontier' or a dict with the keys name / " + " / ".join(_DEFAULTS) + " expected")
    if x.get("name") == "nbp" and len(x) == 1:
        return None
    if x.get("name") != NAME:
        raise ValueError(f"policy: unknown policy {x.get('name')!r} (known: 'nbp', 'frontier')")
    unknown = sorted(set(x) - set(_DEFAULTS) - {"name"}, key=str)
    if unknown:
        raise ValueError(f"policy: unknown keys {unknown}")
    out = {"name": NAME}
    for k, lo, hi in (("radius", 1, MAX_RADIUS), ("dilate", 0, MAX_DILATE), ("distance_penalty", 0, (1 << 20))):
        v = x.get(k, _DEFAULTS[k])
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f"policy: {k} must be an integer in {lo}..{hi}, got {v!r}")
        out[k] = int(v)
    v = x.get("unknown", _DEFAULTS["unknown"])
    if v not in UNKNOWN_MODES:
        raise ValueError(f"policy: unknown must be one of {UNKNOWN_MODES}, got {v!r}")
    out["unknown"] = v
    return {k: out[k] for k in ("name", "radius", "dilate", "unknown", "distance_penalty")}


def _spec(radius, dilate, unknown, distance_penalty):
    return option_spec({"name": NAME, "radius": radius, "dilate": dilate, "unknown": unknown, "distance_penalty": distance_penalty})


def in_sector(h, dy, dx):
    """Is the offset (dy, dx) (integers or integer arrays) in the sector of heading h?"""
    ur, uc = DIRECTIONS[h]
    dy, dx = np.asarray(dy, np.int64), np.asarray(dx, np.int64)
    t = dy * ur + dx * uc
    s = np.abs(dx * ur - dy * uc)
    return (t > 0) & ((s + t) ** 2 < 2 * t * t)


def sector_table(radius):
    """bool [8, 2R+1, 2R+1]: entry [h, dy + R, dx + R] = the offset is non-zero, inside the disc of radius R and in sector h."""
    R = int(radius)
    d = np.arange(-R, R + 1, dtype=np.int64)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    disc = (dy * dy + dx * dx <= R * R) & ((dy != 0) | (dx != 0))
    return np.stack([disc & in_sector(h, dy, dx) for h in range(8)])


def _check_maps(m):
    m = np.asarray(m)
    if m.ndim != 3 or m.shape[0] != 6 or m.shape[1] != m.shape[2] or m.shape[1] < 64 or m.shape[1] % 64:
        raise ValueError(f"frontier: one map stack [6,S,S] with S a multiple of 64 expected, got shape {m.shape}")
    return m


def _shift(a, dr, dc, fill=False):
    """out[r][c] = a[r - dr][c - dc], `fill` where the source lies outside the array."""
    S = a.shape[0]
    out = np.full_like(a, fill)
    r0, r1 = max(dr, 0), min(S + dr, S)
    c0, c1 = max(dc, 0), min(S + dc, S)
    out[r0:r1, c0:c1] = a[r0 - dr:r1 - dr, c0 - dc:c1 - dc]
    return out


def cell_classes(m, dilate=2):
    """maps6 [6,S,S] -> dict of bool [S,S] planes: seen, occupied, free, near_d, seen_d, unknown, frontier."""
    m = _check_maps(m)
    d = _spec(1, dilate, "free", 0)["dilate"]
    S = m.shape[1]
    domain = np.zeros((S, S), bool)
    domain[1:, 1:] = True
    seen = domain & (m[:5] > 0).any(0)
    occupied = domain & (m[5] > 0)
    free = seen & ~occupied
    near_d = np.zeros((S, S), bool)
    for dr in range(-d, d + 1):
        for dc in range(-d, d + 1):
            near_d |= _shift(seen, dr, dc)
    seen_d = np.ones((S, S), bool)
    for dr in range(-d, d + 1):
        for dc in range(-d, d + 1):
            seen_d &= _shift(near_d | ~domain, dr, dc, fill=True)
    unknown = domain & ~seen_d
    near = _shift(unknown, 1, 0) | _shift(unknown, -1, 0) | _shift(unknown, 0, 1) | _shift(unknown, 0, -1)
    return {"seen": seen, "occupied": occupied, "free": free, "near_d": near_d, "seen_d": seen_d, "unknown": unknown, "frontier": free & near}


def gain(frontier, radius=24):
    """bool [S,S] frontier plane -> int64 [8,V,V]: the frontier pixels in each cell's eight disc sectors."""
    f = np.asarray(frontier, bool)
    S = f.shape[0]
    V, R = S // 4, int(radius)
    pad = np.zeros((S + 2 * R, S + 2 * R), np.int64)
    pad[R:R + S, R:R + S] = f
    table = sector_table(R)
    out = np.zeros((8, V, V), np.int64)
    for h in range(8):
        for iy, ix in zip(*np.nonzero(table[h])):             # (the pixel at offset (iy - R, ix - R) from pixel 4 g)
            out[h] += pad[iy:iy + S:4, ix:ix + S:4]
    return out


def policy(m, radius=24, dilate=2, unknown="free", distance_penalty=0):
    """maps6 [6,S,S] -> (out1 float32 [8,V,V], out2 float32 [1,S,S])."""
    m = _check_maps(m)
    sp = _spec(radius, dilate, unknown, distance_penalty)
    cls = cell_classes(m, sp["dilate"])
    V = m.shape[1] // 4
    g = np.arange(V, dtype=np.int64)
    ring = np.maximum(np.abs(g - V // 2)[:, None], np.abs(g - V // 2)[None, :])
    out1 = np.maximum(gain(cls["frontier"], sp["radius"]) - sp["distance_penalty"] * ring[None], 0).astype(np.float32)
    out2 = (cls["unknown"] if sp["unknown"] == "obstacle" else np.zeros_like(cls["unknown"])).astype(np.float32)[None]
    return out1, out2


def policy_batch(maps6, **options):
    """maps6 [B,6,S,S] -> (out1 [B,8,V,V], out2 [B,1,S,S])."""
    outs = [policy(m, **options) for m in np.asarray(maps6)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def pack_bits(plane):
    """bool [..., S, S] -> uint64 [..., S, S/64]: bit i of word w of a row is column 64 w + i (the kernels' packed form)."""
    p = np.asarray(plane, bool)
    S = p.shape[-1]
    b = np.packbits(p.reshape(*p.shape[:-1], S // 64, 64), axis=-1, bitorder="little")
    return np.ascontiguousarray(b).view("<u8").reshape(*p.shape[:-1], S // 64)


def unpack_bits(words, S):
    """The inverse of pack_bits."""
    w = np.ascontiguousarray(np.asarray(words, "<u8"))
    return np.unpackbits(w.view(np.uint8).reshape(*w.shape, 8), axis=-1, bitorder="little").reshape(*w.shape[:-1], S).astype(bool)
