"""A triangle mesh out of the TSDF volume of utility/tsdf.py, by naive surface nets (Gibson 1998): the definition of record (numpy,
no torch).

Not in the reference.  tsdf.extract hands back the zero crossings on the volume's grid edges, a cloud.  This
module puts a surface over exactly those crossings: one vertex per grid cell that holds a crossing, one quad (two triangles) per
crossing edge, no case table.  Every quad corresponds to one row of the fused cloud.

A crossing (v, a) is tsdf.extract's: voxel v = (i, j, k), axis a, the neighbour one step up a inside the volume, both usable
(tsdf.usable_mask) and (S0 < 0) != (S1 < 0); its point is extract's point, the same bits.  All arithmetic is fp32 with one rounding
per operation, no contraction, unless stated.

Cells.   Cell (i, j, k), 0 <= i <= nx - 2 and so on, has the voxels (i + {0,1}, j + {0,1}, k + {0,1}) as corners and the linear
         index of its low corner, (i ny + j) nz + k.  A volume with a dimension of 1 has no cells.  A cell's twelve edges are
         numbered e = 4 a + 2 beta + gamma: a the edge's axis, b < c the other two axes in ascending order, the edge's low voxel
         the cell's corner plus beta along b plus gamma along c.
Vertices.  A cell is active if one of its edges is a crossing.  Its vertex, per coordinate: +0.0, plus the crossing points in edge
         order e = 0 .. 11 (sequentially), divided by f32(count).  Vertices come in cell linear order; a cell's vertex id is its
         rank among the active cells.
Faces.   The crossings in extract's order (voxel linear index, then axis).  (b, c) = ((a + 1) % 3, (a + 2) % 3), the CYCLIC pair.
         The four cells around the edge have their low corners at v + ob e_b + oc e_c, (ob, oc) in {-1, 0}^2; all four exist iff
         1 <= v[b] <= dims[b] - 2 and 1 <= v[c] <= dims[c] - 2.  Otherwise the crossing lies on the volume's boundary and emits
         nothing (it counts in `crossings`, not in `quads`).  The quad is the ring of the cells (-1,-1), (0,-1), (0,0), (-1,0): as
         it stands if S0 < 0 -- its normal is +a, towards positive signed distance (free space) -- else q0, q3, q2, q1.  Ring r0 ..
         r3 gives the triangles (r0, r1, r2) and (r0, r2, r3): quad n (its rank among the emitting crossings) owns face rows 2 n and
         2 n + 1.  int32 (the 2^28-voxel limit keeps ids below 2^31).
Area.    area2 of a face = f32(0.25) dot(n, n), n = cross(v1 - v0, v2 - v0), with surface_metrics' dot and cross; the mesh's area is
         the sum of sqrt(area2) in float64, in face order.

Surface nets puts ONE vertex into a cell even where two sheets of the surface pass through it.  On such ambiguous configurations,
and on the single-sheet maze walls that DESIGN.md 4q describes (a wall seen from both sides: two crossings a voxel apart), the mesh
can be non-manifold: an edge with more than two faces, a vertex shared by two sheets.  Nothing here repairs that.

The device path is csrc/nbp_tsdf_mesh.hip through hipops.tsdf_mesh / TSDFVolume.mesh / FusedMeshMetrics, bit for bit `mesh`.
`mesh_scalar` is the plain transcription with nested loops, what `mesh` is tested against."""
from __future__ import annotations

import collections

import numpy as np

from . import recon_metrics, surface_metrics, tsdf

f32 = np.float32
RING = ((-1, -1), (0, -1), (0, 0), (-1, 0))          # (ob, oc) of a quad's four cells, in ring order
RAW_COUNTS = ("vertices", "faces", "quads", "crossings")
RAW_HEAD = len(RAW_COUNTS) + 1                       # raw vector: the four counts, the area, then completeness and accuracy

Mesh = collections.namedtuple("Mesh", "verts faces area2 quads crossings")


def enabled(spec):
    """Whether the normalised `fusion` spec (tsdf.option_spec) asks for the mesh."""
    return spec is not None and bool(spec.get("mesh"))


def metric_options(surface_spec):
    """The thresholds, cap and cell the fused mesh is judged with: the normalised `surface_metrics` spec, or that option's defaults
    where it is off (the way `fusion` borrows recon_metrics')."""
    return dict(surface_spec or surface_metrics.option_spec(True))


# ---- the crossings, dense
def crossings(vol, lo, voxel, min_weight):
    """-> (M bool [3, nx, ny, nz], P float32 [3, nx, ny, nz, 3]): M[a][v] = (v, a) is a crossing, P[a][v] its point where it is
    one (anything elsewhere)."""
    vol = np.asarray(vol)
    dims = vol.shape[:3]
    use = tsdf.usable_mask(vol, min_weight)
    S, W = vol[..., 0], vol[..., 1]
    neg = S < 0
    with np.errstate(all="ignore"):
        D = S.astype(f32) / W.astype(f32)
    cx, cy, cz = tsdf.axis_centres(lo, voxel, dims)
    centres = np.stack([a.astype(f32) for a in np.broadcast_arrays(cx[:, None, None], cy[None, :, None], cz[None, None, :])], -1)
    M = np.zeros((3, *dims), bool)
    P = np.empty((3, *dims, 3), f32)
    for a in range(3):
        P[a] = centres
        if dims[a] < 2:
            continue
        s0 = tuple(slice(0, -1) if b == a else slice(None) for b in range(3))
        s1 = tuple(slice(1, None) if b == a else slice(None) for b in range(3))
        m = use[s0] & use[s1] & (neg[s0] != neg[s1])
        M[a][s0] = m
        with np.errstate(all="ignore"):
            t = np.where(m, D[s0] / (D[s0] - D[s1]), f32(0))
        P[a][s0 + (a,)] = centres[s0 + (a,)] + t * f32(voxel)
    return M, P


def _axes(a):
    """The other two axes of a, ascending."""
    return [b for b in range(3) if b != a]


def face_area2(verts, faces):
    """float32 [F]: f32(0.25) dot(n, n), n = cross(v1 - v0, v2 - v0) (surface_metrics' dot and cross)."""
    verts = np.asarray(verts, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    v0, v1, v2 = (tuple(verts[faces[:, k], d] for d in range(3)) for k in range(3))
    with np.errstate(all="ignore"):
        n = surface_metrics._cross(surface_metrics._sub(v1, v0), surface_metrics._sub(v2, v0))
        out = f32(0.25) * surface_metrics._dot(n, n)
    out = np.asarray(out, f32).reshape(-1)
    assert out.dtype == f32
    return out


def area_of(area2):
    """The mesh's area: the sum of sqrt(area2) in float64, in face order."""
    return float(np.sqrt(np.asarray(area2, f32).astype(np.float64)).sum())


def mesh(vol, lo, voxel, min_weight):
    """-> Mesh(verts float32 [V,3], faces int32 [F,3], area2 float32 [F], quads = F / 2, crossings = len(tsdf.extract(...)))."""
    vol = np.asarray(vol)
    dims = vol.shape[:3]
    M, P = crossings(vol, lo, voxel, min_weight)
    n_cross = int(M.sum())
    if min(dims) < 2:
        return Mesh(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), np.zeros(0, f32), 0, n_cross)
    C = tuple(d - 1 for d in dims)
    acc = np.zeros((*C, 3), f32)
    cnt = np.zeros(C, np.int32)
    for a in range(3):
        b, c = _axes(a)
        for beta in (0, 1):
            for gamma in (0, 1):
                off = [0, 0, 0]
                off[b], off[c] = beta, gamma
                sl = tuple(slice(off[d], off[d] + C[d]) for d in range(3))
                mk = M[a][sl]
                acc = np.where(mk[..., None], acc + P[a][sl], acc)
                cnt += mk
    active = cnt > 0
    verts = acc[active] / cnt[active].astype(f32)[:, None]
    assert verts.dtype == f32
    ids = np.full(dims, -1, np.int64)
    ids[:C[0], :C[1], :C[2]][active] = np.arange(verts.shape[0])
    lin = np.arange(dims[0] * dims[1] * dims[2]).reshape(dims)
    keys, rings = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        inner = np.zeros(dims, bool)
        sl = [slice(None)] * 3
        sl[b], sl[c] = slice(1, dims[b] - 1), slice(1, dims[c] - 1)
        inner[tuple(sl)] = True
        ijk = np.argwhere(M[a] & inner)
        if not len(ijk):
            continue
        q = []
        for ob, oc in RING:
            cell = ijk.copy()
            cell[:, b] += ob
            cell[:, c] += oc
            q.append(ids[cell[:, 0], cell[:, 1], cell[:, 2]])
        q = np.stack(q, 1)
        assert (q >= 0).all()
        flip = ~(vol[ijk[:, 0], ijk[:, 1], ijk[:, 2], 0] < 0)
        q[flip] = q[flip][:, [0, 3, 2, 1]]
        keys.append(lin[ijk[:, 0], ijk[:, 1], ijk[:, 2]] * 3 + a)
        rings.append(q)
    if not keys:
        return Mesh(np.ascontiguousarray(verts), np.zeros((0, 3), np.int32), np.zeros(0, f32), 0, n_cross)
    r = np.concatenate(rings)[np.argsort(np.concatenate(keys), kind="stable")]
    faces = np.ascontiguousarray(np.stack([r[:, [0, 1, 2]], r[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32))
    return Mesh(np.ascontiguousarray(verts), faces, face_area2(verts, faces), len(r), n_cross)


# ---- the plain transcription: nested loops, one cell, one crossing and one operation at a time
def _crossing_scalar(vol, ijk, a, lo, voxel, min_weight):
    """The point of the crossing (ijk, a) as three fp32 scalars, or None where there is none."""
    dims = vol.shape[:3]
    if ijk[a] + 1 >= dims[a]:
        return None
    nb = tuple(ijk[b] + (1 if b == a else 0) for b in range(3))
    S0, W0 = int(vol[ijk][0]), int(vol[ijk][1])
    S1, W1 = int(vol[nb][0]), int(vol[nb][1])
    if not tsdf._usable_scalar(S0, W0, min_weight) or not tsdf._usable_scalar(S1, W1, min_weight) or (S0 < 0) == (S1 < 0):
        return None
    D0, D1 = f32(S0) / f32(W0), f32(S1) / f32(W1)
    t = f32(D0 / f32(D0 - D1))
    p = [lo[b] + f32((f32(ijk[b]) + f32(0.5)) * voxel) for b in range(3)]
    p[a] = f32(p[a] + f32(t * voxel))
    return p


def _area2_scalar(v0, v1, v2):
    u = [f32(v1[k] - v0[k]) for k in range(3)]
    w = [f32(v2[k] - v0[k]) for k in range(3)]
    with np.errstate(all="ignore"):
        n = [f32(f32(u[1] * w[2]) - f32(u[2] * w[1])), f32(f32(u[2] * w[0]) - f32(u[0] * w[2])), f32(f32(u[0] * w[1]) - f32(u[1] * w[0]))]
        return f32(f32(0.25) * f32(f32(f32(n[0] * n[0]) + f32(n[1] * n[1])) + f32(n[2] * n[2])))


def mesh_scalar(vol, lo, voxel, min_weight):
    vol = np.asarray(vol)
    lo, voxel = np.asarray(lo, f32).reshape(3), f32(voxel)
    dims = vol.shape[:3]
    verts, ids = [], {}
    n_cross = 0
    for i in range(dims[0]):
        for j in range(dims[1]):
            for k in range(dims[2]):
                n_cross += sum(_crossing_scalar(vol, (i, j, k), a, lo, voxel, min_weight) is not None for a in range(3))
    for i in range(dims[0] - 1):
        for j in range(dims[1] - 1):
            for k in range(dims[2] - 1):
                acc, cnt = [f32(0), f32(0), f32(0)], 0
                for e in range(12):
                    a, beta, gamma = e // 4, (e // 2) % 2, e % 2
                    b, c = _axes(a)
                    low = [i, j, k]
                    low[b] += beta
                    low[c] += gamma
                    p = _crossing_scalar(vol, tuple(low), a, lo, voxel, min_weight)
                    if p is None:
                        continue
                    acc = [f32(acc[d] + p[d]) for d in range(3)]
                    cnt += 1
                if cnt:
                    ids[(i, j, k)] = len(verts)
                    verts.append([f32(acc[d] / f32(cnt)) for d in range(3)])
    faces, area2 = [], []
    for i in range(dims[0]):
        for j in range(dims[1]):
            for k in range(dims[2]):
                v = (i, j, k)
                for a in range(3):
                    if _crossing_scalar(vol, v, a, lo, voxel, min_weight) is None:
                        continue
                    b, c = (a + 1) % 3, (a + 2) % 3
                    if not (1 <= v[b] <= dims[b] - 2 and 1 <= v[c] <= dims[c] - 2):
                        continue
                    q = []
                    for ob, oc in RING:
                        cell = list(v)
                        cell[b] += ob
                        cell[c] += oc
                        q.append(ids[tuple(cell)])
                    r = q if int(vol[v][0]) < 0 else [q[0], q[3], q[2], q[1]]
                    for tri in ((r[0], r[1], r[2]), (r[0], r[2], r[3])):
                        faces.append(tri)
                        area2.append(_area2_scalar(*(verts[t] for t in tri)))
    return Mesh(np.asarray(verts, f32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(area2, f32).reshape(-1),
                len(faces) // 2, n_cross)


# ---- the fused mesh against the GT, and the record
def volume_box(lo, voxel, dims, cap):
    """The box of the triangle grid over a fused mesh: the volume's bounds lo .. lo + f32(dims) voxel (fp32) grown by cap.  Every
    vertex is a mean of points between voxel centres, so it lies inside."""
    lo = np.asarray(lo, f32).reshape(3)
    hi = lo + np.asarray(dims, np.int64).astype(f32) * f32(voxel)
    return recon_metrics.grown_box(lo, hi, cap)


def cap_row(n_gt, thresholds, cap):
    """Completeness' (sums, counts) where the mesh has no face: every GT point is `cap` away (d2 = fl(cap cap) for each)."""
    return recon_metrics.stats_reference(np.full(int(n_gt), f32(cap) * f32(cap), f32), thresholds)


def pack_raw(vertices, faces, quads, crossings, area, comp_sums, comp_counts, n_gt, acc_raw):
    """One rollout's raw numbers as ONE float64 vector [5 + (3 + T) + (3 + T)]: the four counts, the area, completeness as sum
    sqrt(d2), sum d2, n_gt and T counts, then surface_metrics.pack_raw of the vertices against the GT mesh (counts below 2^53 are
    exact): what travels between ranks."""
    return np.concatenate([np.array([vertices, faces, quads, crossings, area], np.float64),
                           surface_metrics.pack_raw(comp_sums, comp_counts, n_gt), np.asarray(acc_raw, np.float64).reshape(-1)])


def raw_width(n_thresholds):
    return RAW_HEAD + 2 * (surface_metrics.RAW_HEAD + int(n_thresholds))


def summarise_raw(raw, spec, options=None):
    """pack_raw's vector and the thresholds / cap / cell it was made with (metric_options) -> the record's "fusion_mesh" block,
    JSON-safe: vertices, faces, quads, crossings, area, completeness = {n_gt, cap, completeness_mean, completeness_rmse, thresholds:
    [{threshold, recall}]}, accuracy = surface_metrics.summarise_raw's dict over the vertices, options = {thresholds, cap, cell,
    fusion: the volume's options}.  A ratio without a denominator is None."""
    thresholds, cap = spec["thresholds"], spec["cap"]
    raw = np.asarray(raw, np.float64).reshape(-1)
    T = len(thresholds)
    per = surface_metrics.RAW_HEAD + T
    if raw.shape[0] != raw_width(T):
        raise ValueError(f"fusion mesh: a raw vector of {raw_width(T)} numbers expected, got {raw.shape[0]}")
    out = {key: int(v) for key, v in zip(RAW_COUNTS, raw)}
    out["area"] = float(raw[RAW_HEAD - 1])
    comp = surface_metrics.summarise_raw(raw[RAW_HEAD:RAW_HEAD + per], thresholds, cap)
    out["completeness"] = {"n_gt": comp["n_points"], "cap": comp["cap"], "completeness_mean": comp["accuracy_mean"],
                           "completeness_rmse": comp["accuracy_rmse"],
                           "thresholds": [{"threshold": t["threshold"], "recall": t["precision"]} for t in comp["thresholds"]]}
    out["accuracy"] = surface_metrics.summarise_raw(raw[RAW_HEAD + per:], thresholds, cap)
    out["options"] = {"thresholds": [float(t) for t in thresholds], "cap": float(cap), "cell": float(spec["cell"])}
    if options is not None:
        out["options"]["fusion"] = dict(options)
    return out


def reference_raw(vol, lo, voxel, min_weight, gt, gt_verts, gt_faces, thresholds=surface_metrics.DEFAULT_THRESHOLDS,
                  cap=surface_metrics.DEFAULT_CAP, fused=None):
    """pack_raw's vector entirely in numpy.  gt [G,3]: the GT sample (completeness: GT -> fused mesh, brute force over its triangles
    inside volume_box); gt_verts / gt_faces: the GT mesh (accuracy: the fused mesh's vertices -> GT mesh, surface_metrics.
    reference_raw).  fused: mesh(...)'s result where the caller has it already."""
    ts, cap, _ = surface_metrics.check_options(thresholds, cap)
    vol = np.asarray(vol)
    m = mesh(vol, lo, voxel, min_weight) if fused is None else fused
    gt = np.asarray(gt, f32).reshape(-1, 3)
    if len(m.faces):
        blo, bhi = volume_box(lo, voxel, vol.shape[:3], cap)
        sums, counts = recon_metrics.stats_reference(surface_metrics.mesh_dist2_reference(gt, m.verts, m.faces, blo, bhi, cap), ts)
    else:
        sums, counts = cap_row(len(gt), ts, cap)
    acc = surface_metrics.reference_raw(m.verts, gt_verts, gt_faces, ts, cap)
    return pack_raw(len(m.verts), len(m.faces), m.quads, m.crossings, area_of(m.area2), sums, counts, len(gt), acc)


def reference_block(vol, lo, voxel, min_weight, gt, gt_verts, gt_faces, thresholds=surface_metrics.DEFAULT_THRESHOLDS,
                    cap=surface_metrics.DEFAULT_CAP, cell=surface_metrics.DEFAULT_CELL, options=None, fused=None):
    """The whole "fusion_mesh" block from a volume on the host."""
    ts, cap, cell = surface_metrics.check_options(thresholds, cap, cell)
    raw = reference_raw(vol, lo, voxel, min_weight, gt, gt_verts, gt_faces, ts, cap, fused)
    return summarise_raw(raw, {"thresholds": ts, "cap": cap, "cell": cell}, options)


# ---- PLY, binary little-endian: `float` vertices, `int` face lists
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, verts, faces):
    verts = np.ascontiguousarray(np.asarray(verts, f32).reshape(-1, 3)).astype("<f4")
    faces = np.asarray(faces).reshape(-1, 3)
    rows = np.empty(len(faces), _FACE)
    rows["n"], rows["v"] = 3, faces
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(verts.tobytes())
        fh.write(rows.tobytes())


def read_ply(path):
    """-> (verts float32 [V,3], faces int32 [F,3]) of a file in write_ply's layout (triangles only); ValueError on anything else."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if end < 0 or not data.startswith(b"ply\n"):
        raise ValueError("read_ply: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("read_ply: binary_little_endian 1.0 expected")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    if props != ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]:
        raise ValueError("read_ply: float x y z vertices and uchar / int face lists expected")
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    body = end + len(b"end_header\n")
    if len(data) != body + 12 * nv + _FACE.itemsize * nf:
        raise ValueError("read_ply: the body's length does not fit the header")
    verts = np.frombuffer(data, "<f4", 3 * nv, body).reshape(nv, 3).astype(f32)
    rows = np.frombuffer(data, _FACE, nf, body + 12 * nv)
    if nf and not (rows["n"] == 3).all():
        raise ValueError("read_ply: triangles expected")
    return np.ascontiguousarray(verts), np.ascontiguousarray(rows["v"].astype(np.int32))
