"""Seeded cases shared by tests/test_surface_metrics_host.py and tests/test_gpu_surface.py: point / triangle families, random
meshes with their queries, a tessellated box, and the numpy transcription of the grid walk of csrc/nbp_surface.hip."""
import numpy as np

from nextbestpath_amd.utility import surface_metrics as sm

f32 = np.float32


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _perp(rng, d):
    e = rng.normal(size=d.shape)
    e -= (e * d).sum(1, keepdims=True) * d
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def families(rng, n):
    """{name: (p, a, b, c)} fp32 [n,3] each: the families DESIGN.md 4r's error table is measured on."""
    out = {}
    o = rng.uniform(-30, 30, (n, 3))                                   # small: edges ~0.3 in a 60-unit scene, the query within ~1
    a, b, c = (o + rng.uniform(-0.3, 0.3, (n, 3)) for _ in range(3))
    out["small"] = (o + rng.normal(0, 0.5, (n, 3)), a, b, c)
    a, b, c = (rng.uniform(-50, 50, (n, 3)) for _ in range(3))         # large: edges up to ~100
    out["large"] = (rng.uniform(-60, 60, (n, 3)), a, b, c)
    a, d = rng.uniform(-30, 30, (n, 3)), _unit(rng, n)                 # slivers: 0.5 - 5 long, 1e-3 - 1e-2 of that wide
    L, e = rng.uniform(0.5, 5, (n, 1)), _perp(rng, d)
    b = a + L * d
    c = a + rng.uniform(0, 1, (n, 1)) * L * d + L * rng.uniform(1e-3, 1e-2, (n, 1)) * e
    out["sliver"] = (a + rng.uniform(0, 1, (n, 1)) * L * d + rng.normal(0, 1.0, (n, 3)), a, b, c)
    a, d = rng.uniform(-30, 30, (n, 3)), rng.normal(size=(n, 3))       # degenerate: a point thrice, three points on a line
    kind = rng.integers(0, 3, (n, 1))
    b = np.where(kind == 0, a, a + d * rng.uniform(0.1, 10, (n, 1)))
    c = np.where(kind == 0, a, np.where(kind == 1, b, a + (b - a) * rng.uniform(-1, 2, (n, 1))))
    out["degenerate"] = (a + rng.normal(0, 2.0, (n, 3)), a, b, c)
    a, b, c = (rng.uniform(-50, 50, (n, 3)) for _ in range(3))         # near: 0.03 off the interior of large triangles
    w = rng.dirichlet((1, 1, 1), n)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    out["near"] = (w[:, 0:1] * a + w[:, 1:2] * b + w[:, 2:3] * c + 0.03 * nrm * rng.choice([-1, 1], (n, 1)), a, b, c)
    return {k: tuple(x.astype(f32) for x in v) for k, v in out.items()}


def long_slivers_on_face(rng, n):
    """The family outside any such bound: 40 long, 0.01 wide, the query on the face."""
    a, d = rng.uniform(-30, 30, (n, 3)), _unit(rng, n)
    b = a + 40 * d
    c = a + rng.uniform(0, 40, (n, 1)) * d + 0.01 * _perp(rng, d)
    w = rng.dirichlet((1, 1, 1), n)
    return tuple(x.astype(f32) for x in (w[:, 0:1] * a + w[:, 1:2] * b + w[:, 2:3] * c, a, b, c))


def error_in_units(p, a, b, c):
    """-> (NaNs, worst |sqrt(d2_fp32) - sqrt(d2_fp64)|, the worst of that over 2^-24 (|p - a| + max(|ab|, |ac|)))."""
    d32 = sm.point_triangle_d2(p, a, b, c)
    err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(sm.point_triangle_d2_f64(p, a, b, c)))
    P, A, B, C = (x.astype(np.float64) for x in (p, a, b, c))
    scale = np.linalg.norm(P - A, axis=1) + np.maximum(np.linalg.norm(B - A, axis=1), np.linalg.norm(C - A, axis=1))
    return int(np.isnan(d32).sum()), float(err.max()), float((err / (2.0 ** -24 * scale)).max())


def random_mesh(seed, n_tri, extent, edge):
    """n_tri triangles with centres in [0, extent]^3 and edges up to ~edge -> (verts fp32 [3 n, 3], faces int32 [n, 3])."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0, extent, (n_tri, 1, 3))
    v = (o + rng.uniform(-edge, edge, (n_tri, 3, 3)) * rng.uniform(0.05, 1, (n_tri, 1, 1))).reshape(-1, 3)
    return v.astype(f32), np.arange(3 * n_tri, dtype=np.int32).reshape(-1, 3)


def queries(seed, verts, faces, lo, hi, cap, cell, n):
    """n queries fp32 around a mesh: on its surface, 0.02 off it, anywhere in the box (empty cells among them), outside the grid
    within and beyond R = ceil(cap / cell) cells, at 1e6, and with a NaN."""
    rng = np.random.default_rng(seed)
    verts, faces = np.asarray(verts, f32), np.asarray(faces)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    good = faces[sm.participating(verts, faces, lo.astype(f32), hi.astype(f32))]
    out = []
    k = max(1, n // 6)
    if len(good):
        tri = verts[good[rng.integers(0, len(good), 2 * k)]].astype(np.float64)
        w = rng.dirichlet((1, 1, 1), 2 * k)[:, :, None]
        w[: k // 4] = np.array([1.0, 0.0, 0.0])[None, :, None]          # on a vertex
        w[k // 4: k // 2, 2] = 0.0                                       # on an edge
        w /= w.sum(1, keepdims=True)
        on = (w * tri).sum(1)
        nrm = np.cross(tri[k:, 1] - tri[k:, 0], tri[k:, 2] - tri[k:, 0])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        out += [on[:k], on[k:] + 0.02 * nrm]
    out.append(rng.uniform(lo, hi, (k, 3)))
    R = float(np.ceil(cap / cell))
    for reach in (0.5 * R * cell, (R + 0.5) * cell * 1.001, (R + 2) * cell * 1.001):       # outside: within R, just beyond, beyond
        p = rng.uniform(lo, hi, (k // 2 + 1, 3))
        axis, side = rng.integers(0, 3, len(p)), rng.integers(0, 2, len(p))
        p[np.arange(len(p)), axis] = np.where(side == 0, lo[axis] - reach, hi[axis] + reach)
        out.append(p)
    far = rng.uniform(lo, hi, (4, 3))
    far[0, 0], far[1, 1], far[2, 2], far[3] = 1e6, -1e6, 1e30, [np.nan, far[3, 1], far[3, 2]]
    out.append(far)
    q = np.concatenate(out)
    q = q[rng.permutation(len(q))]
    reps = -(-n // len(q))
    return np.concatenate([q] * reps)[:n].astype(f32)


def box_mesh(side, pitch, origin=(0.0, 0.0, 0.0)):
    """The surface of an axis-aligned cube tessellated into right triangles of leg `pitch` -> (verts fp32, faces int32)."""
    k = int(round(side / pitch))
    g = np.linspace(0.0, side, k + 1)
    verts, faces = [], []
    for axis in range(3):
        for plane in (0.0, side):
            u, v = np.meshgrid(g, g, indexing="ij")
            pts = np.zeros((k + 1, k + 1, 3))
            pts[..., axis], pts[..., (axis + 1) % 3], pts[..., (axis + 2) % 3] = plane, u, v
            base = sum(len(x) for x in verts)
            idx = base + np.arange((k + 1) * (k + 1)).reshape(k + 1, k + 1)
            verts.append(pts.reshape(-1, 3))
            q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
            faces.append(np.stack([q00, q10, q11], -1).reshape(-1, 3))
            faces.append(np.stack([q00, q11, q01], -1).reshape(-1, 3))
    return (np.concatenate(verts) + np.asarray(origin)).astype(f32), np.concatenate(faces).astype(np.int32)


def points_on_mesh(seed, verts, faces, n):
    """n points on the triangles of an axis-aligned mesh, exactly in their planes (the constant coordinate is copied)."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts, f32)[np.asarray(faces)[rng.integers(0, len(faces), n)]].astype(np.float64)
    w = rng.dirichlet((1, 1, 1), n)[:, :, None]
    p = (w * tri).sum(1).astype(f32)
    flat = (tri.max(1) == tri.min(1))
    return np.where(flat, tri[:, 0].astype(f32), p)


def walk_reference(q, verts, faces, lo, hi, cap, cell):
    """The grid walk of csrc/nbp_surface.hip, transcribed: the second, independent statement of its exit rule.  Every
    participating triangle is registered in the cells between the cells of its box's corners; a query visits the shells of cells at
    Chebyshev distance r = r0 .. R = ceil(cap / cell) around its unclamped cell, evaluates what is registered there, and stops after
    shell r once best <= fl(r cell)^2.  -> fp32 [Q], to equal mesh_dist2_reference in every bit."""
    q, verts = np.asarray(q, f32).reshape(-1, 3), np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    lo = np.asarray(lo, f32)
    n, inv = sm.grid_dims(lo, hi, cell)
    keep, c0, c1 = sm.cell_ranges(verts, faces, lo, hi, cell)
    tri = verts[faces[keep]]
    pair_cell, pair_tri = [], []
    for t in range(len(tri)):
        for i in range(c0[t, 0], c1[t, 0] + 1):
            for j in range(c0[t, 1], c1[t, 1] + 1):
                for k in range(c0[t, 2], c1[t, 2] + 1):
                    pair_cell.append((i, j, k))
                    pair_tri.append(t)
    pair_cell = np.asarray(pair_cell, np.int64).reshape(-1, 3)
    pair_tri = np.asarray(pair_tri, np.int64)
    R = int(np.ceil(float(f32(cap)) / float(f32(cell))))
    cap2 = f32(cap) * f32(cap)
    out = np.full(len(q), cap2, f32)
    for m in range(len(q)):
        with np.errstate(all="ignore"):
            fc = np.floor((q[m] - lo) * inv)
        if not np.all((fc >= f32(-R)) & (fc <= (n - 1 + R).astype(f32))):       # beyond reach, or a NaN: cap2, nothing visited
            continue
        c = fc.astype(np.int64)
        cheb = np.abs(pair_cell - c).max(1) if len(pair_cell) else np.zeros(0, np.int64)
        best = cap2
        for r in range(int(max(0, (-c).max(), (c - (n - 1)).max())), R + 1):
            sel = pair_tri[cheb == r]
            if len(sel):
                d = sm.point_triangle_d2(q[m], tri[sel, 0], tri[sel, 1], tri[sel, 2])
                best = np.fmin(best, np.fmin.reduce(d))
            rw = f32(r) * f32(cell)
            if best <= rw * rw:
                break
        out[m] = best
    return out
