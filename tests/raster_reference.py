"""float64 arbiter for the rasteriser and the mesh ray queries, and the seam scenes both are pinned on.

Plain numpy; nothing here comes from oracle/ or from the package, so a mistake in the fp32 plane-form algebra that oracle/raster.py
shares with csrc/nbp_sim.hip shows up against this file.  depth64 casts one ray per pixel centre against every face with
Moeller-Trumbore in float64 and sorts each (pixel, face) pair into SURE (a hit with a margin TAU in the barycentrics and at the clip
plane), POSSIBLE (within TAU of an edge or of the clip plane, or a grazing ray) or a miss; a pixel is AMBIGUOUS when a possible face
could be its winner.  The fp32 code is held to the float64 answer on every pixel that is not ambiguous.

Accuracy statement of the fp32 plane-form algebra (tests/test_raster_reference_host.py): on every non-ambiguous hit pixel
    |z32 - z64| / z64 <= K_DEPTH * cond * 2^-24,
    cond = |e1||v0||e2| / |e2 . (e1 x v0)| + |e1||e2||d| / |(e1 x e2) . d|            (cond64; d = the pixel's ray (dx, dy, 1)).
MEASURED_DEPTH_CONSTANT = 2.81 is max err / (cond 2^-24) of oracle/raster.py::raster_zbuf against depth64 over every frame of every
seam scene of this file and of the four triangle soups (CPU only; neither side is code under test; the worst frame is the third of
soup 1, the seam scenes stay below 1.91); K_DEPTH = 16 is four times that, rounded up to a power of two.  The margin is for seeds
not tried; the algebra has about a dozen roundings between the vertices and z.
"""
import numpy as np

f32 = np.float32
TAN_HALF_FOV = f32(np.tan(np.deg2rad(30.0)))
Z_CLIP = 0.5
TAU = 1e-4          # margin in the barycentrics and (relative) at the clip plane and between depths
KAPPA = 1e-4        # grazing: |det| < KAPPA sum_i |e1_i p_i|
DEGENERATE = 1e-9   # |e1 x e2| <= DEGENERATE |e1||e2|: the face never hits

MEASURED_DEPTH_CONSTANT = 2.81    # measured, see the docstring
K_DEPTH = 16.0                    # 4 x 2.81 = 11.24, rounded up to a power of two
AMBIGUOUS_SHARE_CAP = 0.01


# ---------------------------------------------------------------------------------------------------------------- the arbiter
def _view64(verts, R, T):
    return np.asarray(verts, np.float64) @ np.asarray(R, np.float64) + np.asarray(T, np.float64)


def _rays64(H, W, tan_half_fov):
    s, t = min(H, W), float(f32(tan_half_fov))
    dx = (W - (2.0 * np.arange(W) + 1.0)) / s * t
    dy = (H - (2.0 * np.arange(H) + 1.0)) / s * t
    DX, DY = np.meshgrid(dx, dy)
    return DX.reshape(-1), DY.reshape(-1)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _norm(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _cast(v0, e1, e2, dx, dy, z_clip):
    """Ray (dx, dy, 1) from the origin against triangles (v0, v0 + e1, v0 + e2); v0, e1, e2 are triples of arrays that broadcast
    against dx, dy.  -> z, sure, possible, zp (the depth a possible face competes with: -inf for a grazing one)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        n = _cross(e1, e2)
        alive = _norm(n) > DEGENERATE * _norm(e1) * _norm(e2)
        p = (dy * e2[2] - e2[1], e2[0] - dx * e2[2], dx * e2[1] - dy * e2[0])            # p = d x e2
        a0, a1, a2 = e1[0] * p[0], e1[1] * p[1], e1[2] * p[2]
        det = a0 + a1 + a2
        grazing = (np.abs(det) < KAPPA * (np.abs(a0) + np.abs(a1) + np.abs(a2))) | (det == 0.0)
        inv = 1.0 / det
        u = -(v0[0] * p[0] + v0[1] * p[1] + v0[2] * p[2]) * inv                            # tvec = origin - v0 = -v0
        q = _cross(e1, v0)                                                                 # tvec x e1
        v = (dx * q[0] + dy * q[1] + q[2]) * inv
        z = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv                             # the ray parameter IS z: d_z = 1
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        sure = alive & ~grazing & (m > TAU) & (z > z_clip * (1.0 + TAU))
        possible = alive & ~sure & np.where(grazing, m > -TAU, (m >= -TAU) & (z >= z_clip * (1.0 - TAU)))
        zp = np.where(grazing, -np.inf, z)
    return z, sure, possible, zp


class Depth64:
    """Result of depth64.  z [H,W]: nearest sure depth (inf: none); face: its face (lowest id among equal depths, -1: none); z2, face2:
    the second nearest sure depth; ambiguous [H,W]; the SET of sure / possible winners of a pixel is given as a membership test."""

    def __init__(self, view, faces, H, W, tan_half_fov, z_clip, z, face, z2, face2, ambiguous):
        self._view, self._faces, self.H, self.W, self._t, self._zc = view, faces, H, W, tan_half_fov, z_clip
        self.z, self.face, self.z2, self.face2, self.ambiguous = z, face, z2, face2, ambiguous

    @property
    def hit(self):
        return np.isfinite(self.z)

    def evaluate(self, face_img):
        """face_img [H,W] int (-1: none) -> (z, sure, possible) of THAT face at each pixel."""
        fi = np.asarray(face_img).reshape(-1)
        have = fi >= 0
        tri = self._view[self._faces[np.where(have, fi, 0)]]                               # [P,3,3]
        v0 = tuple(tri[:, 0, k] for k in range(3))
        e1 = tuple(tri[:, 1, k] - tri[:, 0, k] for k in range(3))
        e2 = tuple(tri[:, 2, k] - tri[:, 0, k] for k in range(3))
        dx, dy = _rays64(self.H, self.W, self._t)
        z, sure, possible, zp = _cast(v0, e1, e2, dx, dy, self._zc)
        sh = (self.H, self.W)
        return z.reshape(sh), (sure & have).reshape(sh), (possible & have).reshape(sh), zp.reshape(sh)

    def sure_winner(self, face_img):
        z, sure, _, _ = self.evaluate(face_img)
        return sure & (z < self.z * (1.0 + TAU))

    def possible_winner(self, face_img):
        z, sure, possible, zp = self.evaluate(face_img)
        return (sure & (z < self.z * (1.0 + TAU))) | (possible & (zp < self.z * (1.0 + TAU)))


def depth64(verts, faces, R, T, H, W, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP, chunk=1 << 21):
    """The float64 ray cast of one frame -> Depth64 (see the module docstring for the classification)."""
    view = _view64(verts, R, T)
    faces = np.asarray(faces, np.int64)
    dx, dy = _rays64(H, W, tan_half_fov)
    P, F = dx.shape[0], faces.shape[0]
    dx, dy = dx[:, None], dy[:, None]
    best = np.full((P, 2), np.inf)
    bface = np.full((P, 2), -1, np.int64)
    zp_min = np.full(P, np.inf)
    rows = np.arange(P)
    step = max(1, chunk // P)
    for f0 in range(0, F, step):
        tri = view[faces[f0:f0 + step]]                                                    # [Fc,3,3]
        v0 = tuple(tri[None, :, 0, k] for k in range(3))
        e1 = tuple(tri[None, :, 1, k] - tri[None, :, 0, k] for k in range(3))
        e2 = tuple(tri[None, :, 2, k] - tri[None, :, 0, k] for k in range(3))
        z, sure, possible, zp = _cast(v0, e1, e2, dx, dy, float(z_clip))
        zp_min = np.minimum(zp_min, np.where(possible, zp, np.inf).min(1))
        zs = np.where(sure, z, np.inf)
        cz, cf = [best[:, 0], best[:, 1]], [bface[:, 0], bface[:, 1]]
        for _ in range(2):                                                                 # the chunk's two nearest, lowest id first
            k = zs.argmin(1)
            zk = zs[rows, k]
            cz.append(zk)
            cf.append(np.where(np.isfinite(zk), f0 + k, -1))
            zs[rows, k] = np.inf
        cz, cf = np.stack(cz, 1), np.stack(cf, 1)
        order = np.argsort(cz, axis=1, kind="stable")[:, :2]                               # earlier (lower id) first among equals
        best, bface = np.take_along_axis(cz, order, 1), np.take_along_axis(cf, order, 1)
    sh = (H, W)
    z1 = best[:, 0]
    ambiguous = zp_min < z1 * (1.0 + TAU)
    return Depth64(view, faces, H, W, tan_half_fov, float(z_clip), z1.reshape(sh), bface[:, 0].reshape(sh), best[:, 1].reshape(sh),
                   bface[:, 1].reshape(sh), ambiguous.reshape(sh))


def cond64(verts, faces, R, T, H, W, tan_half_fov, face_img):
    """Condition number of the depth of face face_img[r, c] at pixel (r, c) (module docstring); nan where face_img < 0."""
    view = _view64(verts, R, T)
    fi = np.asarray(face_img).reshape(-1)
    tri = view[np.asarray(faces, np.int64)[np.maximum(fi, 0)]]
    v0 = tuple(tri[:, 0, k] for k in range(3))
    e1 = tuple(tri[:, 1, k] - tri[:, 0, k] for k in range(3))
    e2 = tuple(tri[:, 2, k] - tri[:, 0, k] for k in range(3))
    dx, dy = _rays64(H, W, tan_half_fov)
    d = (dx, dy, np.ones_like(dx))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = _cross(e1, v0)
        n = _cross(e1, e2)
        c = _norm(e1) * _norm(v0) * _norm(e2) / np.abs(e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) + \
            _norm(e1) * _norm(e2) * _norm(d) / np.abs(n[0] * d[0] + n[1] * d[1] + n[2] * d[2])
    return np.where(fi >= 0, c, np.nan).reshape(H, W)


def depth_error_ratio(arb, verts, faces, R, T, z32):
    """err / (cond 2^-24) of an fp32 depth image against the arbiter, on the pixels where both hit; 0 elsewhere.  Where a second sure
    face lies within TAU of the nearest, the fp32 depth may be either's: the smaller ratio counts."""
    z32 = np.asarray(z32, np.float64)
    out = np.full(z32.shape, np.inf)
    for zf, ff in ((arb.z, arb.face), (arb.z2, arb.face2)):
        c = cond64(verts, faces, R, T, arb.H, arb.W, arb._t, ff)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(z32 - zf) / zf / (c * 2.0 ** -24)
        ok = np.isfinite(zf) & (zf < arb.z * (1.0 + TAU))
        out = np.where(ok, np.minimum(out, np.nan_to_num(r, nan=np.inf)), out)
    return np.where(arb.hit & (z32 > 0), out, 0.0)


# ---------------------------------------------------------------------------------------------- float64 segment / triangle test
def segments_hit64(p0, p1, verts, faces, tau=TAU):
    """Does segment p0[i] -> p1[i] hit the mesh strictly inside (0 < t < length)?  -> (hit [n] bool, unsure [n] bool): a face is a sure
    hit with a margin tau in u, v, 1 - u - v and in t / length at both ends, a sure miss when one of them is outside by tau; a segment
    is unsure when no face is a sure hit and some face is neither."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    hit, unsure = np.zeros(len(p0), bool), np.zeros(len(p0), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        alive = np.linalg.norm(np.cross(e1, e2), axis=1) > DEGENERATE * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
        for i in range(len(p0)):
            d = p1[i] - p0[i]
            ln = np.linalg.norm(d)
            if not ln > 0:
                continue
            d = d / ln
            p = np.cross(d[None], e2)
            terms = e1 * p
            det = terms.sum(1)
            grazing = (np.abs(det) < KAPPA * np.abs(terms).sum(1)) | (det == 0)
            tv = p0[i][None] - a
            u = (tv * p).sum(1) / det
            q = np.cross(tv, e1)
            w = (q * d[None]).sum(1) / det
            t = (e2 * q).sum(1) / det / ln
            m = np.minimum(np.minimum(u, w), 1.0 - u - w)
            sure_hit = alive & ~grazing & (m > tau) & (t > tau) & (t < 1.0 - tau)
            sure_miss = ~alive | (m < -tau) | (t < -tau) | (t > 1.0 + tau)
            hit[i] = sure_hit.any()
            unsure[i] = not hit[i] and bool((~sure_miss).any())
    return hit, unsure


# ------------------------------------------------------------------------------------- the device's face boxes, restated (fp32)
def face_boxes32(verts, faces, R, T, H, W, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """Fine-tile box (tx0, tx1, ty0, ty1) that raster_setup_body files each face under, and `have` (False: culled), restated in
    fp32 numpy: the screen box of the part in front of the clip plane, widened by a pixel, clamped to +-1e8 and to the image.  The
    host test uses it to PROVE that a seam scene reaches the path it is named after (list lengths, tile indices)."""
    v = np.asarray(verts, f32)
    R, T = np.asarray(R, f32), np.asarray(T, f32)
    vv = np.stack([((v[:, 0] * R[0, j] + v[:, 1] * R[1, j]) + v[:, 2] * R[2, j]) + T[j] for j in range(3)], 1)
    tri = vv[np.asarray(faces, np.int64)]                                                  # [F,3,3]
    zc, t, s = f32(z_clip), f32(tan_half_fov), f32(min(H, W))
    F = len(tri)
    cmin, cmax = np.full(F, 1e30, f32), np.full(F, -1e30, f32)
    rmin, rmax = np.full(F, 1e30, f32), np.full(F, -1e30, f32)

    def emit(on, x, y, z):
        nonlocal cmin, cmax, rmin, rmax
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            nx, ny = x / (z * t), y / (z * t)
            col = ((f32(W) - s * nx) - f32(1)) * f32(0.5)
            row = ((f32(H) - s * ny) - f32(1)) * f32(0.5)
        cmin = np.where(on, np.fmin(cmin, col), cmin); cmax = np.where(on, np.fmax(cmax, col), cmax)
        rmin = np.where(on, np.fmin(rmin, row), rmin); rmax = np.where(on, np.fmax(rmax, row), rmax)

    for k in range(3):
        a, b = tri[:, k], tri[:, (k + 1) % 3]
        ain, bin_ = a[:, 2] >= zc, b[:, 2] >= zc
        emit(ain, a[:, 0], a[:, 1], a[:, 2])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            tt = (zc - a[:, 2]) / (b[:, 2] - a[:, 2])
            emit(ain != bin_, a[:, 0] + tt * (b[:, 0] - a[:, 0]), a[:, 1] + tt * (b[:, 1] - a[:, 1]), np.full(F, zc, f32))
    behind = (tri[:, :, 2] <= zc).all(1)
    with np.errstate(invalid="ignore"):
        c0 = np.floor(np.fmax(cmin, f32(-1e8))).astype(np.int64) - 1
        c1 = np.ceil(np.fmin(cmax, f32(1e8))).astype(np.int64) + 1
        r0 = np.floor(np.fmax(rmin, f32(-1e8))).astype(np.int64) - 1
        r1 = np.ceil(np.fmin(rmax, f32(1e8))).astype(np.int64) + 1
    c0, r0, c1, r1 = np.maximum(c0, 0), np.maximum(r0, 0), np.minimum(c1, W - 1), np.minimum(r1, H - 1)
    have = ~behind & (cmax >= cmin) & (c0 <= c1) & (r0 <= r1)
    return have, c0 // 8, c1 // 8, r0 // 8, r1 // 8


def coarse_list_counts(verts, faces, R, T, H, W, tan_half_fov=TAN_HALF_FOV, z_clip=Z_CLIP):
    """Entries of every coarse tile's list (8 x 8 fine tiles each), row-major [ctiles_y, ctiles_x], from face_boxes32."""
    have, tx0, tx1, ty0, ty1 = face_boxes32(verts, faces, R, T, H, W, tan_half_fov, z_clip)
    ncx, ncy = -(-(-(-W // 8)) // 8), -(-(-(-H // 8)) // 8)
    out = np.zeros((ncy, ncx), np.int64)
    for cy in range(ncy):
        for cx in range(ncx):
            out[cy, cx] = int((have & (tx0 <= cx * 8 + 7) & (tx1 >= cx * 8) & (ty0 <= cy * 8 + 7) & (ty1 >= cy * 8)).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ scene tools
def look_at(eye, at, up=(0.0, 1.0, 0.0)):
    """Row-vector camera (X_view = X_world R + T) at `eye` looking at `at`: the view axes are the COLUMNS of R.  -> fp32 (R, T)."""
    eye, at, up = np.asarray(eye, np.float64), np.asarray(at, np.float64), np.asarray(up, np.float64)
    z = (at - eye) / np.linalg.norm(at - eye)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    return R.astype(f32), (-(eye @ R)).astype(f32)


def pix_to_view(col, row, z, H, W, tan_half_fov=TAN_HALF_FOV):
    """View-space point at depth z whose projection is pixel (col, row) (fractional; a pixel's centre is its integer index)."""
    s, t = min(H, W), float(f32(tan_half_fov))
    col, row, z = np.broadcast_arrays(np.asarray(col, np.float64), np.asarray(row, np.float64), np.asarray(z, np.float64))
    return np.stack([(W - (2.0 * col + 1.0)) / s * t * z, (H - (2.0 * row + 1.0)) / s * t * z, z], -1)


def to_world(view_pts, R, T):
    """Inverse of X_view = X_world R + T for the fp32 camera (R, T), in float64."""
    return (np.asarray(view_pts, np.float64) - np.asarray(T, np.float64)) @ np.linalg.inv(np.asarray(R, np.float64))


def unshared(tris):
    """[n,3,3] triangles -> (verts [3n,3] fp32, faces [n,3] int32): no vertex is shared, so a face can carry its own flat colour."""
    tris = np.asarray(tris)
    return np.ascontiguousarray(tris.reshape(-1, 3).astype(f32)), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def id_colors(n_faces):
    """One flat colour per face that spells its id: vertex colours [3 n, 3] for `unshared` meshes, k / 256 per byte of the id (the
    barycentric weights of a hit sum to 1 within a few ulp, so the shaded pixel decodes exactly)."""
    i = np.arange(n_faces)
    c = np.stack([i % 256, (i // 256) % 256, i // 65536], 1).astype(f32) / f32(256)
    return np.ascontiguousarray(np.repeat(c, 3, 0))


def decode_ids(rgb, hit, ambient=1.0):
    """Face ids out of an image shaded with id_colors (ambient as rendered); -1 where not hit."""
    k = np.rint(np.asarray(rgb, np.float64) / ambient * 256.0).astype(np.int64)
    return np.where(hit, k[..., 0] + 256 * k[..., 1] + 65536 * k[..., 2], -1)


def _camera(seed):
    rng = np.random.default_rng(1000 + seed)
    eye = rng.uniform(-4, 4, 3)
    d = rng.normal(size=3)
    d[1] *= 0.5
    return look_at(eye, eye + d)


def _nudged(R, T, k):
    """Camera k of a scene designed for camera 0: turned by a few degrees and shifted a little (fp32)."""
    if k == 0:
        return R, T
    a, b = 0.03 * k, -0.02 * k
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (np.asarray(R, np.float64) @ ry @ rx).astype(f32), (np.asarray(T, np.float64) + [0.05 * k, -0.03 * k, 0.1 * k]).astype(f32)


def _tri_px(rng, col, row, size, z, H, W, tilt=0.1):
    """A triangle around pixel (col, row), vertices within `size` pixels of it, at depth z (1 +- tilt) (view space)."""
    c = col + rng.uniform(-size, size, 3)
    r = row + rng.uniform(-size, size, 3)
    return pix_to_view(c, r, z * (1.0 + rng.uniform(-tilt, tilt, 3)), H, W)


def _scene(tris_view, cams, H, W, **extra):
    R, T = cams[0]
    verts, faces = unshared(to_world(np.asarray(tris_view, np.float64).reshape(-1, 3), R, T).reshape(-1, 3, 3))
    return dict(verts=verts, faces=faces, cams=cams, H=H, W=W, **extra)


# ------------------------------------------------------------------------------------------------------------------ seam scenes
def scene_coarse65(seed=65):
    """Second pass of raster_setup_body's coarse-tile loop (`for c0 = 0; c0 < nct; c0 += 64`): it needs more than 64 coarse tiles in a
    frame.  133 x 1412 is 17 x 177 fine tiles = 3 x 23 = 69 coarse tiles, the smallest count above 64 whose tile counts are both odd
    (a half-empty 2 x 2 block on both sides) with W no multiple of 8 and every coarse row cut; coarse tiles 64..68 are the last five
    of the bottom row (rows 128..132, columns >= 1152).  Faces 0..11 lie ONLY in those tiles, face 12 spans the 63|64 boundary, face 13
    covers the whole image (every list, both passes), the other 180 are scattered.  Two frames, so the second pass is also indexed
    by frame."""
    H, W = 133, 1412
    rng = np.random.default_rng(seed)
    tris = [_tri_px(rng, rng.uniform(1162, 1403), 131.2, 1.1, rng.uniform(2, 6), H, W, 0.02) for _ in range(12)]
    tris.append(pix_to_view([1141.0, 1166.0, 1150.0], [130.3, 130.9, 132.4], [3.0, 3.1, 3.05], H, W))
    tris.append(pix_to_view([-3000.0, 4500.0, 700.0], [-400.0, -400.0, 1500.0], [12.0, 12.0, 12.0], H, W))
    for _ in range(180):
        size = rng.choice([3.0, 12.0, 40.0, 150.0], p=[0.3, 0.4, 0.2, 0.1])
        tris.append(_tri_px(rng, rng.uniform(0, W), rng.uniform(0, H), size, rng.uniform(2, 10), H, W))
    c0 = _camera(seed)
    return _scene(tris, [c0, _nudged(*c0, 1)], H, W, only_late=range(12), spanning=12, covering=13)


def _strip(long_axis, seed):
    H, W = (8, 2048) if long_axis == "x" else (2048, 8)
    rng = np.random.default_rng(seed)

    def px(along, across, z):
        return pix_to_view(along, across, z, H, W) if long_axis == "x" else pix_to_view(across, along, z, H, W)
    tris = [px(2043.5 + rng.uniform(-2.4, 2.4, 3), 3.5 + rng.uniform(-3, 3, 3), rng.uniform(2, 4) * np.ones(3)) for _ in range(4)]
    tris.append(px(np.array([-4000.0, 6000.0, 1000.0]), np.array([-60.0, -60.0, 120.0]), 12.0 * np.ones(3)))
    for _ in range(40):
        size = rng.choice([2.0, 6.0, 30.0, 300.0])
        z = rng.uniform(2, 10)
        tris.append(px(rng.uniform(0, 2048) + rng.uniform(-size, size, 3), rng.uniform(0, 8) + rng.uniform(-size, size, 3) * 0.2,
                       z * (1 + rng.uniform(-0.1, 0.1, 3))))
    return _scene(tris, [_camera(seed)], H, W, last_tile=range(4), covering=4)


def scene_wide2048(seed=20):
    """The 8-bit fine-tile box (`tx1 << 8`) at its last value: 8 x 2048 has 256 fine tiles in x, so tile 255 is filed (faces 0..3
    lie in columns 2040..2047 only; face 4 covers the image: tx0 = 0, tx1 = 255).  2048 is the largest width the packing admits
    (2049 is refused); 8 rows are one tile, the least that still renders."""
    return _strip("x", seed)


def scene_tall2048(seed=21):
    """scene_wide2048 transposed: ty1 = 255 sits in the box's top byte (`ty1 << 24`, read back by an unsigned shift)."""
    return _strip("y", seed)


SEG = 16384          # SEG_DEFAULT of nbp_sim.hip: list entries per segment


def scene_seg2(seed=2):
    """Second list segment of raster_block_body (`seg = bx / nblocks`, merged by atomicMin): a coarse list longer than SEG_DEFAULT =
    16384.  72 x 72 is 2 x 2 coarse tiles, the least with other lists beside the long one; 16384 + 700 faces of about 3 pixels
    project inside coarse tile 0 (fine tiles 0..7) at random depths, so the winners of its pixels are spread over both segments,
    and the 12 faces in the other three coarse tiles leave those lists short: their second-segment workgroups take the `s0 >= n`
    exit."""
    H = W = 72
    rng = np.random.default_rng(seed)
    tris = [_tri_px(rng, c, r, 1.3, rng.uniform(2, 10), H, W, 0.02)
            for c, r in zip(rng.uniform(66.5, 69.5, 12), rng.uniform(2, 69.5, 12))]
    tris[4:8] = [_tri_px(rng, c, 68.0, 1.3, rng.uniform(2, 10), H, W, 0.02) for c in rng.uniform(3, 69, 4)]
    n = SEG + 700
    cc, rr, zz = rng.uniform(6, 57, n), rng.uniform(6, 57, n), rng.uniform(2, 10, n)
    for c, r, z in zip(cc, rr, zz):
        tris.append(_tri_px(rng, c, r, 1.5, z, H, W, 0.02))
    return _scene(tris, [_camera(seed)], H, W, long_list=(0, 0))


def scene_small12(seed=12):
    """The 12-face item that shares a batched launch with scene_seg2 (72 x 72): its a.gx_tile has ONE segment while the launch's
    grid has two, so its workgroups beyond gx_tile must return without touching anything."""
    H = W = 72
    rng = np.random.default_rng(seed)
    tris = [_tri_px(rng, rng.uniform(5, 67), rng.uniform(5, 67), 20.0, rng.uniform(2, 10), H, W) for _ in range(12)]
    return _scene(tris, [_camera(seed)], H, W)


PIECE_COUNTS = (64, 65, 255, 256, 257, 319, 320, 321, 640, 641)
PIECE_PLACES = ("first", "last", "boundary")


def scene_pieces(n, place):
    """The piece boundaries of raster_block_body: HITS = 320 block hits per LDS piece (319 / 320 / 321, 640 / 641), 256 list entries
    per round of pass 1 (255 / 256 / 257) and 64 hits per round of pass 2 (64 / 65).  16 x 16 is one 2 x 2 block of fine tiles --
    one workgroup -- and each of the n faces covers it whole, so the list, the block's hits and every tile's hits all count n.
    The nearest face (depth 2, the rest at 3 and beyond) sits at index 0, n - 1, or at the last boundary index below n."""
    H = W = 16
    rng = np.random.default_rng(7 * n + PIECE_PLACES.index(place))
    near = {"first": 0, "last": n - 1, "boundary": max([b for b in (64, 256, 320, 640) if b < n] or [n // 2])}[place]
    depth = 3.0 + 0.01 * rng.permutation(n)
    depth[near] = 2.0
    tris = []
    for z in depth:
        c = np.array([-40.0, 60.0, 8.0]) + rng.uniform(-5, 5, 3)
        r = np.array([-30.0, -30.0, 70.0]) + rng.uniform(-5, 5, 3)
        tris.append(pix_to_view(c, r, z * (1 + rng.uniform(-0.03, 0.03, 3)), H, W))
    return _scene(tris, [_camera(n)], H, W, nearest=near)


TIES_BASE, TIES_COPIES = 128, 12


def scene_ties(seed=5):
    """Equal depths and shared edges: a plane of 8 x 8 quads (two triangles each, 128 faces) facing the camera fills the 32 x 32
    image, and the same 128 faces follow 11 more times under higher ids with the same vertex coordinates, hence the same depth bit
    for bit.  No cracks: every pixel is covered.  The lowest id wins (`fid < fbest`): every winner is below 128.  The copies fill six
    256-thread setup workgroups, so that list entries arrive out of id order; 32 x 32 is four workgroups of tiles."""
    H = W = 32
    gc, gr = np.linspace(-1.37, 33.13, 9), np.linspace(-0.9, 32.6, 9)          # (no grid line through a pixel centre)
    P = pix_to_view(gc[None, :].repeat(9, 0), gr[:, None].repeat(9, 1), 4.0, H, W)        # [9,9,3]
    tris = []
    for j in range(8):
        for i in range(8):
            tris.append([P[j, i], P[j, i + 1], P[j + 1, i + 1]])
            tris.append([P[j, i], P[j + 1, i + 1], P[j + 1, i]])
    sc = _scene(tris, [_camera(seed)], H, W)
    tri = sc["verts"].reshape(-1, 3, 3)
    sc["verts"], sc["faces"] = unshared(np.tile(tri, (TIES_COPIES, 1, 1)))
    return sc


def _needle(through, direction, z, far):
    """A face with one vertex at `far` (coordinates of 1e6 .. 1e7) and two 0.13 apart, 3 units before the view-space point `through`
    (depth z) against `direction`: a strip under a pixel wide that cuts one corner of scene_clip's image, its short edge well outside."""
    c = np.array(through) - 3.0 * np.array(direction)
    perp = np.array([-direction[1], direction[0]]) * (3.0 / 64.0)         # (wider than the diagonal pitch of pixel centres)
    near = [np.round(np.array([*(c + s * perp), z]) * 64) / 64 for s in (1.0, -1.0)]
    return [list(far), list(near[0]), list(near[1])]


def scene_clip():
    """The near plane in raster_setup_body (the all-behind cull, the clipped screen box, its +-1e8 clamp) and in the hit test
    (`z > zclip`).  The camera is a half turn with a dyadic T, so view-space coordinates are exact in fp32: face 0 has all three
    vertices AT z == z_clip (culled: `<=`), face 1 one vertex exactly at z_clip, faces 2..4 straddle the plane (4 with a vertex behind
    the camera), faces 5..7 have a vertex at coordinates of 1e6 and 1e7 (5 in front, 6 behind the camera, 7 on the clip plane: its
    box corner lies beyond 1e8 pixels), face 8 is a wall behind everything and the rest are ordinary.  A face that large has a
    barycentric weight below TAU for its far vertex all over the image, so the arbiter can only call it possible: 5..7 are needles
    (_needle) that win a few corner pixels each, which keeps the frame under the ambiguous-share cap.  48 x 80: the size of the soup
    tests, 6 x 10 tiles."""
    H, W = 48, 80
    R = np.diag([-1.0, 1.0, -1.0]).astype(f32)
    T = np.array([1.0, -2.0, 3.0], f32)
    tris = [
        [[0.0, 0.0, 0.5], [0.03125, 0.0, 0.5], [0.0, 0.03125, 0.5]],
        [[0.125, 0.25, 0.5], [1.0, 0.0, 1.5], [0.0, 1.0, 1.5]],
        [[-1.0, -1.0, 0.25], [1.5, -0.5, 2.0], [0.0, 1.0, 1.0]],
        [[-2.0, 0.5, 0.375], [-1.0, 1.5, 3.0], [-2.5, 1.0, 2.0]],
        [[2.0, 1.0, -3.0], [-2.0, 0.5, 3.0], [1.0, -1.0, 2.5]],
        _needle((5.5, 3.2), (1.0, -1.0), 6.0, (1.0e6, -1.0e6, 5.0)),
        _needle((-6.4, 3.7), (-1.0, -1.0), 7.0, (-1.0e6, -1.0e6, -4.0)),
        _needle((-5.5, -3.2), (-1.0, 1.0), 6.0, (-1.0e7, 1.0e7, 0.5)),
        [[-40.0, -40.0, 8.0], [40.0, -40.0, 8.0], [0.0, 60.0, 8.0]],
    ]
    rng = np.random.default_rng(48)
    for _ in range(20):
        tris.append(np.round(_tri_px(rng, rng.uniform(0, W), rng.uniform(0, H), 9.0, rng.uniform(1, 6), H, W, 0.2) * 64) / 64)
    view = np.asarray(tris, np.float64)
    world = (view - T.astype(np.float64)) @ R.astype(np.float64)                            # R is its own inverse; exact
    verts, faces = unshared(world)
    assert np.array_equal(verts.astype(np.float64).reshape(-1, 3, 3), world)
    return dict(verts=verts, faces=faces, cams=[(R, T)], H=H, W=W, culled=0, at_clip=1)


def scene_frames(n_frames=8, seed=8):
    """MAX_CAMS = 8 cameras in one call's kernel arguments (9 are refused): 60 faces in a ball seen from eight sides, 24 x 40 (3 x 5
    tiles: an odd tile count both ways at the least cost per frame)."""
    H, W = 24, 40
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2, 2, (60, 1, 3))
    tri = c + rng.normal(0, 1, (60, 3, 3)) * rng.choice([0.3, 1.0, 3.0], (60, 1, 1))
    verts, faces = unshared(tri)
    cams = []
    for _ in range(n_frames):
        eye = rng.normal(size=3)
        eye = 7.0 * eye / np.linalg.norm(eye)
        cams.append(look_at(eye, rng.uniform(-0.5, 0.5, 3)))
    return dict(verts=verts, faces=faces, cams=cams, H=H, W=W)


def soup(seed):
    """The random triangle soup of test_raster_random_triangle_soup_vs_oracle (faces crossing the clip plane, behind the camera,
    degenerate, needle-thin and screen-filling), 48 x 80 -> scene dict with `poses` (position, (elevation, azimuth)) in place of
    cameras: the caller turns them into (R, T) with the project's own camera_RT."""
    rng = np.random.default_rng(seed)
    n = 300
    c = rng.uniform(-6, 6, (n, 1, 3))
    size = rng.choice([0.05, 0.5, 3.0, 30.0], (n, 1, 1), p=[0.2, 0.4, 0.3, 0.1])
    tri = (c + rng.normal(0, 1, (n, 3, 3)) * size).astype(np.float32)
    tri[:5, 2] = tri[:5, 1]                                   # degenerate faces
    tri[5:10, :, 1] = tri[5:10, :1, 1]                        # faces in a plane through ... (flat in y)
    verts = tri.reshape(-1, 3)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    poses = [(rng.uniform(-3, 3, 3).tolist(), [float(rng.uniform(-60, 60)), float(rng.uniform(0, 360))]) for _ in range(4)]
    return dict(verts=verts, faces=faces, poses=poses, H=48, W=80)


def seam_scenes():
    """(tag, builder) of every seam scene, in the order of the issue's table; builders are deterministic."""
    out = [("coarse65", scene_coarse65), ("wide2048", scene_wide2048), ("tall2048", scene_tall2048), ("seg2", scene_seg2),
           ("small12", scene_small12)]
    out += [(f"pieces{n}-{p}", (lambda n=n, p=p: scene_pieces(n, p))) for n in PIECE_COUNTS for p in PIECE_PLACES]
    out += [("ties", scene_ties), ("clip", scene_clip), ("frames", scene_frames)]
    return out
