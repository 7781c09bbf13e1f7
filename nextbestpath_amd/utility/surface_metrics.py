"""Accuracy of a reconstructed cloud against the GT MESH, not a sample of it: the definition of record (numpy, no torch).

Not in the reference.  utility/recon_metrics.py measures cloud -> GT sample, and the sample's spacing is that
metric's floor.  The mesh is on the device already, so the distance from a point to the SURFACE can be had exactly:
a truncated point-to-triangle distance, minimised over the mesh.  The device path (csrc/nbp_surface.hip through hipops.MeshPlan /
mesh_dist2 / SurfaceMetrics) equals the functions here bit for bit.

Arithmetic: fp32, one rounding per operation, no contraction.  dot(u, v) = (u0 v0 + u1 v1) + u2 v2; cross(u, v) = (u1 v2 - u2 v1,
u2 v0 - u0 v2, u0 v1 - u1 v0).  min(x, y) is `y if y < x else x`, max(x, y) is `y if y > x else x` (so a NaN operand on the right
never wins): with these every expression below has one value, whatever its operands.

point_triangle_d2(p, a, b, c) = max(core, box):
  core  the minimum, in this order, of the three segment candidates (a, b), (b, c), (c, a) and, where admitted, the face candidate.
        Segment (u, v): uv = v - u, up = p - u, den = dot(uv, uv), num = dot(up, uv), t = num / den if den > 0 else 0, clamped to
        [0, 1] (t = max(t, 0), then min(t, 1)), e = up - t uv, candidate dot(e, e).
        Face: ab = b - a, ac = c - a, ap = p - a, n = cross(ab, ac), nn = dot(n, n); admitted iff nn > GUARD (dot(ab, ab) dot(ac, ac))
        and dot(n, cross(ab, ap)) >= 0 and dot(n, cross(c - b, p - b)) >= 0 and dot(n, cross(a - c, p - c)) >= 0; candidate
        (h h) / nn with h = dot(ap, n).  A degenerate triangle (a point, a line) has nn = 0: the face is never admitted, nothing
        divides by zero, and the value is the distance to that point or segment.
  box   the squared distance from p to the triangle's fp32 bounding box: lo = min(min(a, b), c), hi = max(max(a, b), c) per axis,
        e = max(max(lo - p, p - hi), 0), value (e0 e0 + e1 e1) + e2 e2.  In exact arithmetic it never exceeds the true distance; it
        is there so that the device's early exit is provable without a bound on triangle size or on core's rounding error
        (csrc/nbp_surface.hip's header).

GUARD = 2^-24 is the relative size of |n|^2 = |ab|^2 |ac|^2 sin^2 below which the plane's normal is not trusted and the edges alone
speak; the choice is measured on the CPU (every guard from 0 to 2^-20 gives the same error on ordinary triangles, 2^-16
and above drop large triangles with one small angle, and 2^-24 is the largest at which nothing measured differs from no guard)."""
from __future__ import annotations

import math

import numpy as np

from . import recon_metrics

f32 = np.float32
GUARD = f32(2.0 ** -24)
MAX_THRESHOLDS = recon_metrics.MAX_THRESHOLDS
DEFAULT_THRESHOLDS = (0.05, 0.1, 0.25, 0.5, 1.0)     # conventions, not measurements: a coarse distribution from 4q's 0.03 to the
DEFAULT_CAP = 5.0                                    # coverage radius; cap and cell are recon_metrics' own
DEFAULT_CELL = 1.0
MAX_AXIS = 2048                                      # csrc/nbp_recon.hip: cells per axis, and 2^28 cells in all
RAW_HEAD = 3                                         # raw vector: sum sqrt(d2), sum d2, n, then T counts


# ---- the options
def check_options(thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP, cell=DEFAULT_CELL):
    """-> (thresholds as a tuple of floats, cap, cell); ValueError on anything the kernels would refuse."""
    try:
        return recon_metrics.check_options(thresholds, cap, cell)
    except ValueError as e:
        raise ValueError(str(e).replace("recon metrics", "surface metrics")) from None


def option_spec(option):
    """The planning option `surface_metrics` -> None (off) or the keyword dict of hipops.SurfaceMetrics: None / False = off, True =
    the defaults, a dict with any of `thresholds` (1 to 8, positive, finite, <= cap), `cap` and `cell`."""
    if option is None or option is False:
        return None
    if option is True:
        option = {}
    if not isinstance(option, dict) or set(option) - {"thresholds", "cap", "cell"}:
        raise ValueError("surface_metrics: None, True or a dict with the keys thresholds / cap / cell expected")
    ts, cap, cell = check_options(option.get("thresholds", DEFAULT_THRESHOLDS), option.get("cap", DEFAULT_CAP),
                                  option.get("cell", DEFAULT_CELL))
    return {"thresholds": ts, "cap": cap, "cell": cell}


def mesh_box(verts_host, cap):
    """The box of the triangle grid: the bounds of the finite vertices grown by cap, in fp32 -> (lo, hi).  Every finite vertex is
    inside it, so every triangle of finite vertices takes part; a query outside it is farther than cap from the surface."""
    v = np.asarray(verts_host, f32).reshape(-1, 3)
    v = v[np.all(np.isfinite(v), axis=1)]
    if v.shape[0] < 1:
        raise ValueError("surface metrics: a mesh without a finite vertex")
    return recon_metrics.grown_box(v.min(0), v.max(0), cap)


# ---- point to triangle
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


def _segment(p, u, v):
    uv, up = _sub(v, u), _sub(p, u)
    den, num = _dot(uv, uv), _dot(up, uv)
    pos = den > 0
    t = np.where(pos, num / np.where(pos, den, f32(1)), f32(0))
    t = _min(_max(t, f32(0)), f32(1))
    e = (up[0] - t * uv[0], up[1] - t * uv[1], up[2] - t * uv[2])
    return _dot(e, e)


def point_triangle_d2(p, a, b, c):
    """Squared distance from p to the triangle a b c (module docstring), fp32.  p, a, b, c: [..., 3], broadcast against each other."""
    p, a, b, c = (np.asarray(x, f32) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    p, a, b, c = (tuple(x[..., k] for k in range(3)) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        core = _segment(p, a, b)
        core = _min(core, _segment(p, b, c))
        core = _min(core, _segment(p, c, a))
        ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
        n = _cross(ab, ac)
        nn = _dot(n, n)
        ok = nn > GUARD * (_dot(ab, ab) * _dot(ac, ac))
        ok = ok & (_dot(n, _cross(ab, ap)) >= 0)
        ok = ok & (_dot(n, _cross(_sub(c, b), _sub(p, b))) >= 0)
        ok = ok & (_dot(n, _cross(_sub(a, c), _sub(p, c))) >= 0)
        h = _dot(ap, n)
        face = (h * h) / np.where(ok, nn, f32(1))
        core = np.where(ok, _min(core, face), core)
        e = []
        for k in range(3):
            lo, hi = _min(_min(a[k], b[k]), c[k]), _max(_max(a[k], b[k]), c[k])
            e.append(_max(_max(lo - p[k], p[k] - hi), f32(0)))
        box = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        out = _max(core, box)
    assert out.dtype == f32
    return out


def _segment_scalar(p, u, v):
    uv = [f32(v[k] - u[k]) for k in range(3)]
    up = [f32(p[k] - u[k]) for k in range(3)]
    den = f32(f32(f32(uv[0] * uv[0]) + f32(uv[1] * uv[1])) + f32(uv[2] * uv[2]))
    num = f32(f32(f32(up[0] * uv[0]) + f32(up[1] * uv[1])) + f32(up[2] * uv[2]))
    t = f32(num / den) if den > 0 else f32(0)
    if f32(0) > t:
        t = f32(0)
    if f32(1) < t:
        t = f32(1)
    e = [f32(up[k] - f32(t * uv[k])) for k in range(3)]
    return f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2]))


def point_triangle_d2_scalar(p, a, b, c):
    """point_triangle_d2 for ONE point and ONE triangle, an operation at a time on numpy fp32 scalars (what the vectorised
    function is tested against, and what the kernel transcribes)."""
    p, a, b, c = ([f32(x) for x in np.asarray(v, f32).reshape(3)] for v in (p, a, b, c))

    def dot(u, v):
        return f32(f32(f32(u[0] * v[0]) + f32(u[1] * v[1])) + f32(u[2] * v[2]))

    def cross(u, v):
        return [f32(f32(u[1] * v[2]) - f32(u[2] * v[1])), f32(f32(u[2] * v[0]) - f32(u[0] * v[2])),
                f32(f32(u[0] * v[1]) - f32(u[1] * v[0]))]

    def sub(u, v):
        return [f32(u[k] - v[k]) for k in range(3)]

    with np.errstate(all="ignore"):
        core = _segment_scalar(p, a, b)
        for u, v in ((b, c), (c, a)):
            s = _segment_scalar(p, u, v)
            if s < core:
                core = s
        ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
        n = cross(ab, ac)
        nn = dot(n, n)
        if (nn > f32(GUARD * f32(dot(ab, ab) * dot(ac, ac))) and dot(n, cross(ab, ap)) >= 0
                and dot(n, cross(sub(c, b), sub(p, b))) >= 0 and dot(n, cross(sub(a, c), sub(p, c))) >= 0):
            h = dot(ap, n)
            face = f32(f32(h * h) / nn)
            if face < core:
                core = face
        e = []
        for k in range(3):
            lo = b[k] if b[k] < a[k] else a[k]
            lo = c[k] if c[k] < lo else lo
            hi = b[k] if b[k] > a[k] else a[k]
            hi = c[k] if c[k] > hi else hi
            m, m2 = f32(lo - p[k]), f32(p[k] - hi)
            m = m2 if m2 > m else m
            e.append(f32(0) if f32(0) > m else m)
        box = f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2]))
    return box if box > core else core


def point_triangle_d2_f64(p, a, b, c):
    """The same expression evaluated in float64 on the same fp32 inputs, with GUARD's test left to the fp32 evaluation's degenerate
    case only (nn > 0): the yardstick of the fp32 error, not part of the definition."""
    p, a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)

    def seg(u, v):
        uv, up = v - u, p - u
        den, num = (uv * uv).sum(-1), (up * uv).sum(-1)
        t = np.clip(np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
        e = up - t[..., None] * uv
        return (e * e).sum(-1)

    core = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    ok = ((nn > 0) & ((n * np.cross(ab, ap)).sum(-1) >= 0) & ((n * np.cross(c - b, p - b)).sum(-1) >= 0)
          & ((n * np.cross(a - c, p - c)).sum(-1) >= 0))
    h = (ap * n).sum(-1)
    return np.where(ok, np.minimum(core, h * h / np.where(ok, nn, 1.0)), core)


# ---- point to mesh
def participating(verts, faces, lo, hi):
    """-> bool [F]: the triangles that take part: indices inside [0, V), all three vertices finite and lo <= vertex <= hi on every
    axis, compared in fp32 (a NaN is outside)."""
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(invalid="ignore"):
        vin = np.all(np.isfinite(verts) & (verts >= lo) & (verts <= hi), axis=1)
    inr = np.all((faces >= 0) & (faces < verts.shape[0]), axis=1)
    ok = inr.copy()
    if verts.shape[0]:
        ok[inr] = vin[faces[inr]].all(1)
    return ok


def mesh_dist2_reference(q, verts, faces, lo, hi, cap, chunk=1 << 20):
    """Brute force, fp32: out[i] = min(cap2, min over the participating triangles of point_triangle_d2(q_i, ...)), cap2 = fl(cap cap).
    A query with a NaN or infinite coordinate gets cap2.  `chunk` = point-triangle pairs held in memory at once."""
    q = np.ascontiguousarray(np.asarray(q, f32).reshape(-1, 3))
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    cap2 = f32(cap) * f32(cap)
    tri = verts[faces[participating(verts, faces, lo, hi)]]            # [F', 3, 3]
    out = np.full(q.shape[0], cap2, f32)
    fin = np.all(np.isfinite(q), axis=1)
    if tri.shape[0] == 0 or not fin.any():
        return out
    rows = max(1, int(chunk) // tri.shape[0])
    idx = np.flatnonzero(fin)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    for i0 in range(0, idx.shape[0], rows):
        sel = idx[i0:i0 + rows]
        d = point_triangle_d2(q[sel][:, None, :], a, b, c)
        out[sel] = np.fmin(np.fmin.reduce(d, axis=1), cap2)
    return out


def mesh_dist2_reference_scalar(q, verts, faces, lo, hi, cap):
    """mesh_dist2_reference as nested loops over the scalar transcription."""
    q = np.asarray(q, f32).reshape(-1, 3)
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    cap2 = f32(f32(cap) * f32(cap))
    keep = participating(verts, faces, lo, hi)
    out = np.full(q.shape[0], cap2, f32)
    for i in range(q.shape[0]):
        if not np.all(np.isfinite(q[i])):
            continue
        best = cap2
        for f in np.flatnonzero(keep):
            d = point_triangle_d2_scalar(q[i], *verts[faces[f]])
            if d < best:
                best = d
        out[i] = best
    return out


# ---- the triangle grid (csrc/nbp_recon.hip's grid; csrc/nbp_surface.hip registers a triangle in these cells)
def grid_dims(lo, hi, cell):
    """Cells per axis of the grid over [lo, hi] with cells 1.001 cell wide -> (n [3] int, inv fp32); ValueError beyond the
    kernels' limits (2048 cells on an axis, 2^28 cells)."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    if not np.all(ext >= 0):
        raise ValueError("surface metrics: hi below lo")
    n = (ext / float(f32(cell))).astype(np.int64) + 1
    if np.any(n > MAX_AXIS) or int(np.prod(n)) > 1 << 28:
        raise ValueError("surface metrics: more than 2048 cells on an axis or 2^28 cells")
    return n, f32(1.0 / (float(f32(cell)) * 1.001))


def cell_ranges(verts, faces, lo, hi, cell):
    """-> (keep bool [F], c0 int [F', 3], c1 int [F', 3]): the participating triangles and, for each, the inclusive range of cells it
    is registered in: the cells of its bounding box's two corners (fp32: floor(fl(fl(x - lo) inv)), clamped to the grid)."""
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    lo = np.asarray(lo, f32)
    n, inv = grid_dims(lo, hi, cell)
    keep = participating(verts, faces, lo, hi)
    tri = verts[faces[keep]]
    c0 = np.floor((tri.min(1) - lo) * inv).astype(np.int64)
    c1 = np.floor((tri.max(1) - lo) * inv).astype(np.int64)
    return keep, np.clip(c0, 0, n - 1), np.clip(c1, 0, n - 1)


def plan_counts(verts, faces, lo, hi, cell):
    """-> (faces_used, entries): the participating triangles and the (triangle, cell) pairs of the grid."""
    keep, c0, c1 = cell_ranges(verts, faces, lo, hi, cell)
    return int(keep.sum()), int(np.prod(c1 - c0 + 1, axis=1).sum())


# ---- summary
def pack_raw(sums, counts, n):
    """The raw numbers of one cloud as ONE float64 vector [3 + T] (counts below 2^53 are exact): what travels between ranks."""
    return np.concatenate([np.asarray(sums, np.float64).reshape(2), np.array([n], np.float64),
                           np.asarray(counts, np.float64).reshape(-1)])


def summarise_raw(raw, thresholds, cap):
    """Raw sums and counts -> {n_points, cap, accuracy_mean, accuracy_rmse, thresholds: [{threshold, precision}]}; a ratio without a
    denominator is None (never NaN: the dict goes into JSON)."""
    raw = np.asarray(raw, np.float64).reshape(-1)
    T = len(thresholds)
    if raw.shape[0] != RAW_HEAD + T:
        raise ValueError(f"surface metrics: a raw vector of {RAW_HEAD + T} numbers expected, got {raw.shape[0]}")
    n = int(raw[2])
    return {"n_points": n, "cap": float(cap),
            "accuracy_mean": float(raw[0]) / n if n > 0 else None,
            "accuracy_rmse": math.sqrt(float(raw[1]) / n) if n > 0 else None,
            "thresholds": [{"threshold": float(t), "precision": float(int(raw[RAW_HEAD + k])) / n if n > 0 else None}
                           for k, t in enumerate(thresholds)]}


RECORD_TAIL = ("has_fused", "faces", "faces_used", "entries")     # what follows the two clouds' raw vectors in a record's row


def pack_record(cloud_raw, fused_raw, mesh):
    """One rollout's raw numbers as ONE float64 vector [2 (3 + T) + 4]: pack_raw of the raw cloud, pack_raw of the fused cloud (zeros
    where the rollout has none: fused_raw None), then has_fused and the mesh's faces, faces_used, entries (counts below 2^53 are
    exact): what travels between ranks."""
    cloud_raw = np.asarray(cloud_raw, np.float64).reshape(-1)
    fused = np.zeros_like(cloud_raw) if fused_raw is None else np.asarray(fused_raw, np.float64).reshape(-1)
    if fused.shape != cloud_raw.shape:
        raise ValueError("surface metrics: the two clouds' raw vectors differ in length")
    tail = [0.0 if fused_raw is None else 1.0, mesh["faces"], mesh["faces_used"], mesh["entries"]]
    return np.concatenate([cloud_raw, fused, np.asarray(tail, np.float64)])


def summarise_record(row, spec):
    """pack_record's vector and the normalised options (option_spec) it was made with -> the record's "surface" block, JSON-safe:
    {"cloud": summarise_raw's dict over the whole raw cloud, "fused": the same over the fused cloud (only where there is one),
    "mesh": {faces, faces_used, entries}, "options": {thresholds (a list), cap, cell}}."""
    thresholds, cap = spec["thresholds"], spec["cap"]
    row = np.asarray(row, np.float64).reshape(-1)
    per = RAW_HEAD + len(thresholds)
    if row.shape[0] != 2 * per + len(RECORD_TAIL):
        raise ValueError(f"surface metrics: a record row of {2 * per + len(RECORD_TAIL)} numbers expected, got {row.shape[0]}")
    out = {"cloud": summarise_raw(row[:per], thresholds, cap)}
    if row[2 * per] != 0:
        out["fused"] = summarise_raw(row[per:2 * per], thresholds, cap)
    out["mesh"] = {key: int(v) for key, v in zip(RECORD_TAIL[1:], row[2 * per + 1:])}
    out["options"] = {"thresholds": [float(t) for t in thresholds], "cap": float(cap), "cell": float(spec["cell"])}
    return out


def reference_raw(cloud, verts, faces, thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP):
    ts, cap, _ = check_options(thresholds, cap)
    cloud = np.asarray(cloud, f32).reshape(-1, 3)
    lo, hi = mesh_box(verts, cap)
    sums, counts = recon_metrics.stats_reference(mesh_dist2_reference(cloud, verts, faces, lo, hi, cap), ts)
    return pack_raw(sums, counts, cloud.shape[0])


def reference(cloud, verts, faces, thresholds=DEFAULT_THRESHOLDS, cap=DEFAULT_CAP):
    """The summary entirely in numpy: brute force over the triangles inside mesh_box(verts, cap)."""
    ts, cap, _ = check_options(thresholds, cap)
    return summarise_raw(reference_raw(cloud, verts, faces, ts, cap), ts, cap)
