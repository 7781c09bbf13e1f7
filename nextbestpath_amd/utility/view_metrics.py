"""Held-out view metrics of a rollout's coloured cloud: the definition of record (numpy, no torch).

Not in the reference.  Coverage and the reconstruction metrics measure geometry in 3-D; these ask what a user
of a reconstruction asks first: seen from a place the agent did not stand in, does it look like the scene?  The whole coloured
cloud is point-splatted from held-out lattice poses and compared pixel by pixel with the mesh render of the same poses: how much
of what is visible is filled at the right depth (`view_completeness`), left empty (`hole`), shows a farther surface through a
front surface the cloud lacks (`leak`), hangs in front of the real surface (`floater`), and how far depth and colour are off
where the depth is right (`depth_mae`, `depth_rmse`, `psnr`).

The device path (csrc/nbp_views.hip through hipops.render_cloud / view_stats / ViewMetrics) produces the key buffer and raw counts
and sums only; the ratios are formed here, on the host, from those -- by the same function for the device path and for this
numpy reference, and only after the raw numbers of all views have been added.

Projection of a point p for camera (R, T), all fp32, one rounding per operation: v = p R + T (nbp_sim.hip::to_view's order),
t = v2 tan_half_fov, nx = v0 / t, ny = v1 / t, s = min(H, W), cf = ((f32(W / s) - nx) 0.5) f32(s - 1), col = floor(cf + 0.5), rows
alike from ny and f32(H / s): the inverse of the un-projection's NDC tables (every un-projected pixel projects onto itself), not
of the rasteriser's pixel-centre rule.  A point takes part iff z_clip < v2 < z_far and nx, ny are finite.

The default splat radius of 1 pixel is a convention, not a measurement: nobody has measured which radius suits a cloud thinned
by gathering_factor = 0.05 (tools/bench_views.py prints view_completeness against the radius).  The record carries the options
it was made with."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
TAN_HALF_FOV = f32(np.tan(np.deg2rad(30.0)))
Z_CLIP = 0.5                           # hipops.Z_CLIP: the plane at which the mesh render cuts
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_RADIUS = 4
MAX_POINTS = (1 << 32) - 1             # a cloud must hold fewer points than this (the key's low word is the index)
MAX_PIXELS = 1 << 29
N_HEADINGS = 8
RAW_COUNTS = ("n_gt", "n_c", "n_hit", "n_hole", "n_leak", "n_floater")
RAW_SUMS = ("sum_abs_dz", "sum_dz2", "sum_rgb2")
RAW_WIDTH = len(RAW_COUNTS) + len(RAW_SUMS)
DEFAULTS = {"views": 16, "seed": 0, "radius": 1, "depth_tolerance": 1.0}
_KEYS = {"views", "seed", "radius", "depth_tolerance", "height", "width", "z_far"}


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def option_spec(option):
    """The planning option `view_metrics` -> None (off) or the normalised dict: None / False = off, True = the defaults, a dict with
    any of `views` (16), `seed` (0), `radius` (1 pixel, 0..4), `depth_tolerance` (1.0: the coverage radius's convention), `height` /
    `width` (absent: the camera's) and `z_far` (absent: params.zfar).  Anything else is a ValueError."""
    if option is None or option is False:
        return None
    if option is True:
        option = {}
    if not isinstance(option, dict) or set(option) - _KEYS:
        raise ValueError("view_metrics: None, True or a dict with the keys " + " / ".join(sorted(_KEYS)) + " expected")
    spec = dict(DEFAULTS)
    spec.update(option)
    if not _is_int(spec["views"]) or spec["views"] < 1:
        raise ValueError("view_metrics: views must be a positive integer")
    if not _is_int(spec["seed"]) or spec["seed"] < 0:
        raise ValueError("view_metrics: seed must be a non-negative integer")
    if not _is_int(spec["radius"]) or not 0 <= spec["radius"] <= MAX_RADIUS:
        raise ValueError(f"view_metrics: radius must be an integer in 0..{MAX_RADIUS}")
    if not _is_num(spec["depth_tolerance"]) or not (spec["depth_tolerance"] >= 0 and math.isfinite(spec["depth_tolerance"])):
        raise ValueError("view_metrics: depth_tolerance must be non-negative and finite")
    for k in ("height", "width"):
        if k in spec and (not _is_int(spec[k]) or spec[k] < 2):
            raise ValueError(f"view_metrics: {k} must be an integer of at least 2")
    if "z_far" in spec and (not _is_num(spec["z_far"]) or not (spec["z_far"] > Z_CLIP and math.isfinite(spec["z_far"]))):
        raise ValueError("view_metrics: z_far must be finite and beyond the clip plane")
    out = {"views": int(spec["views"]), "seed": int(spec["seed"]), "radius": int(spec["radius"]),
           "depth_tolerance": float(spec["depth_tolerance"])}
    for k in ("height", "width"):
        if k in spec:
            out[k] = int(spec[k])
    if "z_far" in spec:
        out["z_far"] = float(spec["z_far"])
    return out


def resolved_options(spec, height, width, z_far):
    """A normalised spec with the camera's image size and the parameters' zfar filled in where it leaves them open: the options
    an evaluation is made with, and what its record carries."""
    out = dict(spec)
    out.setdefault("height", int(height))
    out.setdefault("width", int(width))
    out.setdefault("z_far", float(z_far))
    return out


# ---- evaluation poses
def choose_views(nbrs, mesh_hit, start_node, n, seed):
    """-> [(node, heading)]: the lattice positions reachable from `start_node` over the planner's edges that the mesh does not cut
    (a breadth-first search over nbrs[node] = [(neighbour, edge id)] with not mesh_hit[edge id]: every place the agent could ever
    stand), each with each of the 8 headings, in node-then-heading order; from that list `n` are drawn without replacement by
    numpy.random.default_rng(seed) (all of them where there are no more than n).  Independent of the rollout's seed and trajectory:
    two rollouts in one scene from one start are judged from the same places."""
    start_node, n = int(start_node), int(n)
    seen = {start_node}
    queue = [start_node]
    while queue:
        nxt = []
        for a in queue:
            for b, e in nbrs[a]:
                if not mesh_hit[e] and b not in seen:
                    seen.add(int(b))
                    nxt.append(int(b))
        queue = nxt
    pool = [(node, h) for node in sorted(seen) for h in range(N_HEADINGS)]
    if len(pool) <= n:
        return pool
    pick = np.random.default_rng(int(seed)).choice(len(pool), size=n, replace=False)
    return [pool[int(i)] for i in pick]


# ---- projection and splat
def project(points, R, T, H, W, z_clip=Z_CLIP, z_far=np.inf, tan_half_fov=TAN_HALF_FOV):
    """points [n,3] -> (takes_part bool [n], row float32 [n], col float32 [n] (floor(cf + 0.5), not yet an integer: it may be far
    outside the image), v2 float32 [n])."""
    R, T = np.asarray(R, f32).reshape(3, 3), np.asarray(T, f32).reshape(3)
    p = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
    s = min(H, W)
    half, sm1 = f32(0.5), f32(s - 1)
    with np.errstate(all="ignore"):
        v = [((p[:, 0] * R[0, j] + p[:, 1] * R[1, j]) + p[:, 2] * R[2, j]) + T[j] for j in range(3)]
        t = v[2] * f32(tan_half_fov)
        nx, ny = v[0] / t, v[1] / t
        cf = ((f32(W / s) - nx) * half) * sm1
        rf = ((f32(H / s) - ny) * half) * sm1
        col, row = np.floor(cf + half), np.floor(rf + half)
        ok = (v[2] > f32(z_clip)) & (v[2] < f32(z_far)) & np.isfinite(nx) & np.isfinite(ny)
    assert col.dtype == f32 and row.dtype == f32 and v[2].dtype == f32
    return ok, row, col, v[2]


def empty_keys(V, H, W):
    return np.full((V, H, W), EMPTY, np.uint64)


def splat(points, cams, H, W, radius=1, z_far=np.inf, keys=None, first_index=0, z_clip=Z_CLIP, tan_half_fov=TAN_HALF_FOV):
    """Keys uint64 [V,H,W]: per pixel the smallest (float bits of v2) << 32 | point index over the points whose (2 radius + 1)^2
    footprint, clipped to the image, holds the pixel -- the nearest point, the lower index at equal depth; ~0 = empty.  cams [V,12]
    (hipops.cams12).  `keys`: accumulate into an earlier result (a minimum is order-free: a cloud splatted in parts gives the same
    bits as at once); `first_index`: the index of points[0] in the whole cloud."""
    cams = np.asarray(cams, f32).reshape(-1, 12)
    p = np.asarray(points, f32).reshape(-1, 3)
    r = int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"view metrics: radius {radius} outside 0..{MAX_RADIUS}")
    if H * W > MAX_PIXELS or int(first_index) + p.shape[0] >= MAX_POINTS:
        raise ValueError("view metrics: more than 2^29 pixels, or a cloud of 2^32 - 1 points or more")
    V = cams.shape[0]
    keys = empty_keys(V, H, W) if keys is None else keys
    index = np.arange(p.shape[0], dtype=np.uint64) + np.uint64(first_index)
    for c in range(V):
        ok, row, col, z = project(p, cams[c, :9], cams[c, 9:], H, W, z_clip, z_far, tan_half_fov)
        with np.errstate(invalid="ignore"):
            ok = ok & (row >= -r) & (row <= H - 1 + r) & (col >= -r) & (col <= W - 1 + r)
        ri, ci = row[ok].astype(np.int64), col[ok].astype(np.int64)
        key = (z[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[ok]
        flat = keys[c].reshape(-1)
        for dr in range(-r, r + 1):
            for dc in range(-r, r + 1):
                rr, cc = ri + dr, ci + dc
                m = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
                np.minimum.at(flat, rr[m] * W + cc[m], key[m])
    return keys


def resolve(keys, cloud_rgb=None):
    """Keys -> (z_c float32 (-1 where empty), index int64 (-1 where empty), rgb_c float32 [...,3] = cloud_rgb[index] (0 where
    empty) or None)."""
    keys = np.asarray(keys, np.uint64)
    empty = keys == EMPTY
    z = (keys >> np.uint64(32)).astype(np.uint32).view(f32).reshape(keys.shape).copy()
    z[empty] = f32(-1)
    index = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    index[empty] = -1
    rgb = None
    if cloud_rgb is not None:
        rgb = np.zeros(keys.shape + (3,), f32)
        rgb[~empty] = np.asarray(cloud_rgb, f32).reshape(-1, 3)[index[~empty]]
    return z, index, rgb


def classify(z_c, z_gt, depth_tolerance, z_far):
    """Per-pixel classes -> dict of bool arrays gt, c, hit, hole, leak, floater.  gt = the mesh is visible closer than z_far, c =
    the pixel is not empty; the depth comparisons are made in fp32 on z_c - z_gt."""
    z_c, z_gt = np.asarray(z_c, f32), np.asarray(z_gt, f32)
    tau = f32(depth_tolerance)
    gt = (z_gt > f32(-1)) & (z_gt < f32(z_far))
    c = z_c > f32(-1)                                  # (a splatted depth is beyond the clip plane: positive)
    dz = z_c - z_gt
    both = gt & c
    return {"gt": gt, "c": c, "hit": both & (np.abs(dz) <= tau), "hole": gt & ~c, "leak": both & (dz > tau),
            "floater": c & (~gt | (dz < -tau))}


def raw_stats(z_c, rgb_c, z_gt, rgb_gt, depth_tolerance, z_far):
    """[V,H,W] images -> (counts int64 [V,6] = n_gt, n_c, n_hit, n_hole, n_leak, n_floater, sums float64 [V,3] over the hit pixels
    = sum |dz|, sum dz^2, squared colour error summed over the three channels; differences in float64 from the fp32 values; the
    colour sum is 0 where either colour image is missing)."""
    z_c, z_gt = np.asarray(z_c, f32), np.asarray(z_gt, f32)
    V = z_c.shape[0]
    cl = classify(z_c, z_gt, depth_tolerance, z_far)
    counts = np.stack([cl[k].reshape(V, -1).sum(1) for k in ("gt", "c", "hit", "hole", "leak", "floater")], 1).astype(np.int64)
    sums = np.zeros((V, 3), np.float64)
    for v in range(V):
        hit = cl["hit"][v]
        dz = z_c[v][hit].astype(np.float64) - z_gt[v][hit].astype(np.float64)
        sums[v, 0], sums[v, 1] = np.abs(dz).sum(), (dz * dz).sum()
        if rgb_c is not None and rgb_gt is not None:
            d = np.asarray(rgb_c, f32)[v][hit].astype(np.float64) - np.asarray(rgb_gt, f32)[v][hit].astype(np.float64)
            sums[v, 2] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum()
    return counts, sums


def pack_raw(counts, sums):
    """The raw numbers of one evaluation as ONE float64 array [V, 9] (counts below 2^53 are exact): what travels between ranks."""
    counts, sums = np.asarray(counts), np.asarray(sums, np.float64)
    return np.concatenate([counts.reshape(-1, len(RAW_COUNTS)).astype(np.float64), sums.reshape(-1, len(RAW_SUMS))], 1)


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else None


def _psnr(rgb2, n_hit):
    if n_hit <= 0 or not rgb2 > 0:
        return None                                    # no pixel to compare, no colours, or no error at all: never an infinity
    return 10.0 * math.log10(1.0 / (float(rgb2) / (3.0 * float(n_hit))))     # peak 1.0: ambient x vertex colours in [0, 1]


def summarise_raw(raw, options=None):
    """Raw rows [V, 9] -> the metrics, JSON-safe: the rows are added first, then the ratios formed.  view_completeness, hole and
    leak are shares of n_gt, floater of n_c; depth_mae / depth_rmse / psnr over the hit pixels; per_view lists of
    view_completeness and psnr.  A ratio without a denominator is None (never NaN), and so is the PSNR of a zero colour error
    (a cloud without colours gives the depth half only).  `options`: carried along as the block's `options`."""
    raw = np.asarray(raw, np.float64)
    if raw.ndim != 2 or raw.shape[1] != RAW_WIDTH:
        raise ValueError(f"view metrics: raw rows of {RAW_WIDTH} numbers expected, got shape {raw.shape}")
    tot = raw.sum(0) if raw.shape[0] else np.zeros(RAW_WIDTH)
    n_gt, n_c, n_hit, n_hole, n_leak, n_fl = (int(v) for v in tot[:6])
    out = {"n_views": int(raw.shape[0]), "n_gt": n_gt, "n_c": n_c, "n_hit": n_hit,
           "view_completeness": _ratio(n_hit, n_gt), "hole": _ratio(n_hole, n_gt), "leak": _ratio(n_leak, n_gt),
           "floater": _ratio(n_fl, n_c), "depth_mae": _ratio(tot[6], n_hit),
           "depth_rmse": math.sqrt(float(tot[7]) / n_hit) if n_hit > 0 else None, "psnr": _psnr(tot[8], n_hit),
           "per_view": {"view_completeness": [_ratio(int(r[2]), int(r[0])) for r in raw],
                        "psnr": [_psnr(r[8], int(r[2])) for r in raw]}}
    if options is not None:
        out["options"] = dict(options)
    return out


def reference(cloud, cloud_rgb, cams, z_gt, rgb_gt, radius=1, depth_tolerance=1.0, z_far=np.inf, raw=False):
    """The whole evaluation in numpy: splat, resolve, classify, add -> summarise_raw's dict (or the raw rows)."""
    z_gt = np.asarray(z_gt, f32)
    V, H, W = z_gt.shape
    z_c, _, rgb_c = resolve(splat(cloud, cams, H, W, radius, z_far), cloud_rgb)
    rows = pack_raw(*raw_stats(z_c, rgb_c, z_gt, rgb_gt, depth_tolerance, z_far))
    return rows if raw else summarise_raw(rows)
