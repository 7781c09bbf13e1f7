"""Next-best-view by ray-cast information gain as a policy behind the network's interface: the DEFINITION (numpy, CPU) that
csrc/nbp_infogain.hip equals bit for bit.  Not in the reference.

The frontier policy (utility/frontier.py) counts frontier pixels in a value cell's eight disc sectors and looks straight through
walls.  This one counts the UNKNOWN pixels a camera standing on the cell could see: rays leave the cell and stop at the occupancy
evidence the planner already holds, the camera-height band maps6[5].  The cell classes (`occupied`, `unknown` = outside the closing
of `seen` by `dilate`, the domain D of rows and columns >= 1) are utility/frontier.py::cell_classes, the sectors its sector_table.

Blocked.  blocked(p) holds when p lies outside the S x S window, or outside D, or occupied(p).

Ray fan of radius R.  One ray per target offset (ty, tx) with max(|ty|, |tx|) = R: 8 R rays.  Point k = 1..R of a ray has each
coordinate sgn(m) ((2 k |m| + R) // (2 R)), m that coordinate of the target: k m / R rounded half away from zero, in integers.  The
major axis advances by exactly one per point; the fan marks every pixel of the (2 R + 1)-square and its point lists are exactly
D4-symmetric (tests/test_infogain_host.py).

Walk from value cell g at pixel c = (4 g0, 4 g1).  If blocked(c) nothing is visible.  Otherwise every ray starts with prev = c and
takes its points in order; it stops at the first point p with blocked(p), and at the first diagonal step (both coordinates changed)
whose two corner pixels (p.r, prev.c) and (prev.r, p.c) are both blocked -- a ray does not slip between two diagonally touching wall
pixels.  Otherwise p is visible and prev = p.  (The cell's own pixel is not a point of any ray: it is never marked.)

Outputs.  gain(h, g) = the pixels p that are unknown, visible from g and whose offset p - c is in sector_table(R)[h] (non-zero, in
the disc, within 22.5 degrees of the heading).
    out1[h, g0, g1] = float32(max(gain - distance_penalty * max(|g0 - V/2|, |g1 - V/2|), 0))
    out2[0, p]      = the frontier policy's: 1.0 where `unknown` == "obstacle" and unknown(p), else 0.0
Every count is an integer below 2^24: the floats are exact.  Value row 0 and value column 0 sit outside D: their gain is 0.

The defaults (radius 24, dilate 2, unknown "free", distance_penalty 0) are the frontier policy's: conventions, not measurements.
"""
from __future__ import annotations

import functools

import numpy as np

from . import frontier

NAME = "infogain"
MAX_RADIUS, MAX_DILATE = frontier.MAX_RADIUS, frontier.MAX_DILATE
UNKNOWN_MODES = frontier.UNKNOWN_MODES


def option_spec(x):
    """The planning option `policy` for this policy -> the normalised spec: a dict with exactly the keys name ("infogain"), radius
    (1..31), dilate (0..8), unknown ("free" / "obstacle") and distance_penalty (an integer >= 0), the frontier policy's keys, ranges
    and defaults.  "infogain" = the defaults; a dict {"name": "infogain", ...} fills the rest with them.  None, "nbp" and
    {"name": "nbp"} -> None (the network).  ValueError on anything else, the name "frontier" included (that is
    utility/frontier.py::option_spec's; testers/frontier_policy.py::make_policy dispatches on the name)."""
    if x is None or x == "nbp" or (isinstance(x, dict) and x.get("name") == "nbp" and len(x) == 1):
        return None
    if isinstance(x, str):
        x = {"name": x}
    if not isinstance(x, dict):
        raise ValueError("policy: None, 'nbp', 'infogain' or a dict with the keys name / radius / dilate / unknown / distance_penalty expected")
    if x.get("name") != NAME:
        raise ValueError(f"policy: unknown policy {x.get('name')!r} (known here: 'nbp', 'infogain')")
    out = frontier.option_spec(dict(x, name=frontier.NAME))          # the same keys, ranges, defaults and refusals
    out["name"] = NAME
    return out


def _spec(radius, dilate, unknown, distance_penalty):
    return option_spec({"name": NAME, "radius": radius, "dilate": dilate, "unknown": unknown, "distance_penalty": distance_penalty})


@functools.lru_cache(maxsize=None)
def _ray_table(R):
    t = np.arange(-R, R + 1, dtype=np.int64)
    targets = [(-R, x) for x in t[:-1]] + [(y, R) for y in t[:-1]] + [(R, -x) for x in t[:-1]] + [(-y, -R) for y in t[:-1]]
    m = np.asarray(targets, np.int64)                                  # [8 R, 2], clockwise from the top-left corner
    k = np.arange(1, R + 1, dtype=np.int64)[None, :, None]
    pts = np.sign(m)[:, None, :] * ((2 * k * np.abs(m)[:, None, :] + R) // (2 * R))
    pts.setflags(write=False)
    return pts


def ray_table(radius):
    """int64 [8 R, R, 2]: entry [i, k - 1] = point k (d_row, d_col) of ray i.  Ray i ends on its target, entry [i, R - 1]; the
    targets run clockwise round the square's rim from (-R, -R).  Read-only."""
    R = int(radius)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"infogain: radius must be in 1..{MAX_RADIUS}, got {radius!r}")
    return _ray_table(R)


def _blocked_unknown(m, dilate):
    cls = frontier.cell_classes(m, dilate)
    S = cls["occupied"].shape[0]
    domain = np.zeros((S, S), bool)
    domain[1:, 1:] = True
    return cls["occupied"] | ~domain, cls["unknown"]


def _visible_all(blocked, R):
    """bool [S,S] blocked plane -> bool [2R+1, 2R+1, V, V]: entry [dy + R, dx + R, g0, g1] = pixel 4 g + (dy, dx) is visible from
    value cell g.  One numpy step per (ray, point) over all the cells."""
    S = blocked.shape[0]
    V = S // 4
    pad = np.ones((S + 2 * R, S + 2 * R), bool)                        # outside the window: blocked
    pad[R:R + S, R:R + S] = blocked
    at = lambda dy, dx: pad[R + dy:R + dy + S:4, R + dx:R + dx + S:4]  # blocked(4 g + (dy, dx)) for every g
    vis = np.zeros((2 * R + 1, 2 * R + 1, V, V), bool)
    start = ~at(0, 0)
    if not start.any():
        return vis
    for ray in ray_table(R):
        alive = start.copy()
        qy = qx = 0
        for py, px in ray:
            py, px = int(py), int(px)
            stop = at(py, px)
            if py != qy and px != qx:
                stop = stop | (at(py, qx) & at(qy, px))
            alive &= ~stop
            if not alive.any():
                break
            vis[py + R, px + R] |= alive
            qy, qx = py, px
    return vis


def visible(m, dilate=2, radius=24, cells=()):
    """maps6 [6,S,S], cells [n,2] = (g0, g1) -> bool [n, 2R+1, 2R+1]: entry [i, dy + R, dx + R] = pixel 4 g + (dy, dx) is visible
    from cell i."""
    m = frontier._check_maps(m)
    sp = _spec(radius, dilate, "free", 0)
    R, V = sp["radius"], m.shape[1] // 4
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    if len(cells) and (cells.min() < 0 or cells.max() >= V):
        raise ValueError(f"infogain: cells outside 0..{V - 1}")
    vis = _visible_all(_blocked_unknown(m, sp["dilate"])[0], R)
    return np.ascontiguousarray(np.moveaxis(vis[:, :, cells[:, 0], cells[:, 1]], 2, 0))


def gain(blocked, unknown, radius=24):
    """bool [S,S] planes -> int64 [8,V,V]: the unknown pixels visible from each cell in its eight disc sectors."""
    blocked, unknown = np.asarray(blocked, bool), np.asarray(unknown, bool)
    S = blocked.shape[0]
    V, R = S // 4, int(radius)
    vis = _visible_all(blocked, R)
    pad = np.zeros((S + 2 * R, S + 2 * R), bool)
    pad[R:R + S, R:R + S] = unknown
    table = frontier.sector_table(R)
    out = np.zeros((8, V, V), np.int64)
    for h in range(8):
        for iy, ix in zip(*np.nonzero(table[h])):
            out[h] += vis[iy, ix] & pad[iy:iy + S:4, ix:ix + S:4]
    return out


def policy(m, radius=24, dilate=2, unknown="free", distance_penalty=0):
    """maps6 [6,S,S] -> (out1 float32 [8,V,V], out2 float32 [1,S,S])."""
    m = frontier._check_maps(m)
    sp = _spec(radius, dilate, unknown, distance_penalty)
    blocked, unk = _blocked_unknown(m, sp["dilate"])
    V = m.shape[1] // 4
    g = np.arange(V, dtype=np.int64)
    ring = np.maximum(np.abs(g - V // 2)[:, None], np.abs(g - V // 2)[None, :])
    out1 = np.maximum(gain(blocked, unk, sp["radius"]) - sp["distance_penalty"] * ring[None], 0).astype(np.float32)
    out2 = (unk if sp["unknown"] == "obstacle" else np.zeros_like(unk)).astype(np.float32)[None]
    return out1, out2


def policy_batch(maps6, **options):
    """maps6 [B,6,S,S] -> (out1 [B,8,V,V], out2 [B,1,S,S])."""
    outs = [policy(m, **options) for m in np.asarray(maps6)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
