"""TSDF fusion of a rollout's depth frames into a truncated signed distance volume, and the fused surface cloud taken out of it:
the definition of record (numpy, no torch).

Not in the reference.  The raw cloud keeps 5 % of each frame's pixels, every point with its own frame's full
noise.  The volume averages the many frames that see one surface, and a later frame that sees through a point contradicts it.  It
is an observer: nothing of the rollout reads it.

State: ONE int32 array [nx, ny, nz, 2]; voxel (i, j, k) -- linear index (i ny + j) nz + k -- holds (S, W): the sum of its quantised
signed distances and the number of its observations.  The sums are integers: frames may be integrated in any order and in any
grouping and give the same bits (tests/test_tsdf_host.py permutes and regroups them).

All arithmetic is fp32 with one rounding per operation unless stated.  The centre of voxel (i, j, k) on axis a is lo_a + (f32(i_a)
+ 0.5) voxel, the multiply first, then the add.  It is projected with view_metrics.project exactly as that stands.  A frame updates
the voxel iff it takes part there, 0 <= row <= H - 1 and 0 <= col <= W - 1 (decided on the floats), d = depth[row, col] has d > -1
(a NaN is invalid) and d <= max_depth, and sdf = d - v2 >= -trunc; then S += (int) rint(min(sdf, trunc) scale), W += 1, with scale
= f32(127) / f32(trunc) formed once on the host and rint to the nearest even.

The device path is csrc/nbp_tsdf.hip through hipops.tsdf_integrate / tsdf_integrate_batch / tsdf_extract / tsdf_stats / TSDFVolume,
bit for bit these functions.  `*_scalar` below are plain transcriptions with nested loops, what the vectorised functions are tested
against.

The defaults (voxel 0.25, trunc 1.0, min_weight 1) are conventions, not measurements: nobody has measured which voxel size or
truncation suits these scenes.  The record carries the options it was made with."""
from __future__ import annotations

import math

import numpy as np

from . import recon_metrics, view_metrics

f32 = np.float32
QUANT = 127                            # a distance of +-trunc is stored as +-127
MAX_VOXELS = 1 << 28
DEFAULTS = {"voxel": 0.25, "trunc": 1.0, "min_weight": 1}
_KEYS = {"voxel", "trunc", "max_depth", "min_weight", "mesh"}
RAW_TAIL = ("observed_voxels", "usable_voxels", "frames")       # what follows recon_metrics.pack_raw's numbers in a raw row


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def option_spec(option):
    """The planning option `fusion` -> None (off) or the normalised dict: None / False = off, True = the defaults, a dict with any
    of `voxel` (0.25), `trunc` (1.0, at least 2 voxel), `max_depth` (absent: the parameters' sensor_range, the range the
    un-projection keeps), `min_weight` (1, an integer >= 1) and `mesh` (true / false: the triangle mesh of utility/tsdf_mesh.py
    out of the volume at the rollout's end as well; the key is there only when it is on).  Anything else is a ValueError."""
    if option is None or option is False:
        return None
    if option is True:
        option = {}
    if not isinstance(option, dict) or set(option) - _KEYS:
        raise ValueError("fusion: None, True or a dict with the keys " + " / ".join(sorted(_KEYS)) + " expected")
    spec = dict(DEFAULTS)
    spec.update(option)
    if not isinstance(spec.get("mesh", False), bool):
        raise ValueError("fusion: mesh must be true or false")
    for k in ("voxel", "trunc"):
        if not _is_num(spec[k]) or not (spec[k] > 0 and math.isfinite(spec[k])):
            raise ValueError(f"fusion: {k} must be positive and finite")
    if not spec["trunc"] >= 2 * spec["voxel"]:
        raise ValueError("fusion: trunc must be at least 2 voxel (a surface crossing needs a voxel inside the band on either side)")
    if not _is_int(spec["min_weight"]) or spec["min_weight"] < 1:
        raise ValueError("fusion: min_weight must be an integer of at least 1")
    if "max_depth" in spec and (not _is_num(spec["max_depth"]) or not (spec["max_depth"] > 0 and math.isfinite(spec["max_depth"]))):
        raise ValueError("fusion: max_depth must be positive and finite")
    out = {"voxel": float(spec["voxel"]), "trunc": float(spec["trunc"]), "min_weight": int(spec["min_weight"])}
    if "max_depth" in spec:
        out["max_depth"] = float(spec["max_depth"])
    if spec.get("mesh", False):
        out["mesh"] = True
    return out


def resolved_options(spec, sensor_range):
    """A normalised spec with the parameters' sensor_range filled in where it leaves max_depth open: the options a volume is made
    with, and what its record carries."""
    out = dict(spec)
    out.setdefault("max_depth", float(sensor_range))
    return out


def scale_of(trunc):
    """The quantisation scale f32(127) / f32(trunc), formed once on the host."""
    return f32(QUANT) / f32(trunc)


def volume_geometry(bbox, spec):
    """(lo float32 [3], dims int [3]) of the volume of a rollout whose GT bounds are bbox = (lo, hi): the bounds grown by trunc on
    every side, dims = ceil(extent / voxel) in float64 (at least 1).  ValueError above 2^28 voxels."""
    blo, bhi = np.asarray(bbox[0], np.float64).reshape(3), np.asarray(bbox[1], np.float64).reshape(3)
    if not (np.all(np.isfinite(blo)) and np.all(np.isfinite(bhi)) and np.all(bhi >= blo)):
        raise ValueError("fusion: bbox = (lo [3], hi [3]) with finite lo <= hi expected")
    trunc, voxel = float(spec["trunc"]), float(spec["voxel"])
    lo, hi = blo - trunc, bhi + trunc
    dims = np.maximum(np.ceil((hi - lo) / voxel), 1.0)
    if float(dims[0]) * float(dims[1]) * float(dims[2]) > MAX_VOXELS:
        raise ValueError(f"fusion: a volume of {int(dims[0])} x {int(dims[1])} x {int(dims[2])} voxels, above 2^28")
    return lo.astype(f32), dims.astype(np.int64)


def empty_volume(dims):
    return np.zeros((int(dims[0]), int(dims[1]), int(dims[2]), 2), np.int32)


def axis_centres(lo, voxel, dims):
    """Per axis the fp32 centres lo_a + (f32(i) + 0.5) voxel: the multiply first, then the add."""
    lo, voxel = np.asarray(lo, f32).reshape(3), f32(voxel)
    return [lo[a] + (np.arange(int(dims[a])).astype(f32) + f32(0.5)) * voxel for a in range(3)]


def voxel_centres(lo, voxel, dims):
    """The centres of all voxels in linear order, float32 [nx ny nz, 3]."""
    cx, cy, cz = axis_centres(lo, voxel, dims)
    g = np.meshgrid(cx, cy, cz, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], 1).astype(f32)


def integrate(vol, lo, voxel, depth, cam12, trunc, max_depth, z_clip=view_metrics.Z_CLIP, tan_half_fov=view_metrics.TAN_HALF_FOV):
    """One frame depth [H,W] of camera cam12 (R row-major then T) into vol (in place; returned)."""
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    cam = np.asarray(cam12, f32).reshape(12)
    dims = vol.shape[:3]
    ok, row, col, v2 = view_metrics.project(voxel_centres(lo, voxel, dims), cam[:9], cam[9:], H, W, z_clip=z_clip,
                                            tan_half_fov=tan_half_fov)
    trunc, scale = f32(trunc), scale_of(trunc)
    with np.errstate(invalid="ignore"):
        ok = ok & (row >= 0) & (row <= H - 1) & (col >= 0) & (col <= W - 1)
    idx = np.flatnonzero(ok)
    d = depth[row[idx].astype(np.int64), col[idx].astype(np.int64)]
    with np.errstate(invalid="ignore"):
        valid = (d > f32(-1)) & (d <= f32(max_depth))
    idx, d = idx[valid], d[valid]
    sdf = d - v2[idx]
    keep = sdf >= -trunc
    idx, sdf = idx[keep], sdf[keep]
    q = np.rint(np.minimum(sdf, trunc) * scale)
    assert q.dtype == f32
    flat = vol.reshape(-1, 2)
    flat[idx, 0] += q.astype(np.int32)
    flat[idx, 1] += 1
    return vol


def usable_mask(vol, min_weight):
    """W >= min_weight and |S| < 127 W: a saturated voxel (free space that only ever saw a far background, or its mirror image
    behind a surface) carries no surface."""
    S, W = vol[..., 0].astype(np.int64), vol[..., 1].astype(np.int64)
    return (W >= int(min_weight)) & (np.abs(S) < QUANT * W)


def extract(vol, lo, voxel, min_weight):
    """The fused surface cloud float32 [n,3]: for every voxel in linear order and axis 0, 1, 2 in that order, with the neighbour
    one step up that axis inside the volume: both usable and (S0 < 0) != (S1 < 0) -> one point, the voxel's centre with t voxel added
    on that axis, t = D0 / (D0 - D1), D = f32(S) / f32(W).  Output order: (linear index, axis)."""
    dims = vol.shape[:3]
    n = dims[0] * dims[1] * dims[2]
    use = usable_mask(vol, min_weight)
    S, W = vol[..., 0], vol[..., 1]
    neg = S < 0
    with np.errstate(all="ignore"):
        D = S.astype(f32) / W.astype(f32)
    centres = voxel_centres(lo, voxel, dims)
    lin = np.arange(n).reshape(dims)
    keys, pts = [], []
    for a in range(3):
        if dims[a] < 2:
            continue
        s0 = tuple(slice(0, -1) if b == a else slice(None) for b in range(3))
        s1 = tuple(slice(1, None) if b == a else slice(None) for b in range(3))
        m = use[s0] & use[s1] & (neg[s0] != neg[s1])
        v = lin[s0][m]
        d0, d1 = D[s0][m], D[s1][m]
        t = d0 / (d0 - d1)
        p = centres[v].copy()
        p[:, a] = p[:, a] + t * f32(voxel)
        keys.append(v * 3 + a)
        pts.append(p)
    if not keys:
        return np.zeros((0, 3), f32)
    keys, pts = np.concatenate(keys), np.concatenate(pts)
    out = pts[np.argsort(keys, kind="stable")]
    assert out.dtype == f32
    return np.ascontiguousarray(out)


def stats(vol, min_weight):
    """{"observed_voxels": #(W > 0), "usable_voxels": #usable}."""
    return {"observed_voxels": int(np.count_nonzero(vol[..., 1] > 0)), "usable_voxels": int(np.count_nonzero(usable_mask(vol, min_weight)))}


# ---- the plain transcription: nested loops, one voxel and one operation at a time
def _project_scalar(p, cam, H, W, z_clip, tan_half_fov):
    """view_metrics.project for one point -> (takes part, row, col, v2)."""
    R, T = cam[:9], cam[9:]
    v = [f32(f32(f32(p[0] * R[j]) + f32(p[1] * R[3 + j])) + f32(p[2] * R[6 + j])) + T[j] for j in range(3)]
    s = min(H, W)
    with np.errstate(all="ignore"):
        t = v[2] * f32(tan_half_fov)
        nx, ny = v[0] / t, v[1] / t
        col = np.floor(((f32(W / s) - nx) * f32(0.5)) * f32(s - 1) + f32(0.5))
        row = np.floor(((f32(H / s) - ny) * f32(0.5)) * f32(s - 1) + f32(0.5))
    ok = bool(v[2] > f32(z_clip)) and bool(v[2] < f32(np.inf)) and bool(np.isfinite(nx)) and bool(np.isfinite(ny))
    return ok, row, col, v[2]


def integrate_scalar(vol, lo, voxel, depth, cam12, trunc, max_depth, z_clip=view_metrics.Z_CLIP,
                     tan_half_fov=view_metrics.TAN_HALF_FOV):
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    cam = np.asarray(cam12, f32).reshape(12)
    lo, voxel, trunc, max_depth = np.asarray(lo, f32).reshape(3), f32(voxel), f32(trunc), f32(max_depth)
    scale = f32(QUANT) / trunc
    nx, ny, nz = vol.shape[:3]
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                p = [lo[0] + f32((f32(i) + f32(0.5)) * voxel), lo[1] + f32((f32(j) + f32(0.5)) * voxel),
                     lo[2] + f32((f32(k) + f32(0.5)) * voxel)]
                ok, row, col, v2 = _project_scalar(p, cam, H, W, z_clip, tan_half_fov)
                if not ok or not (row >= 0 and row <= H - 1 and col >= 0 and col <= W - 1):
                    continue
                d = depth[int(row), int(col)]
                if not (d > f32(-1) and d <= max_depth):
                    continue
                sdf = f32(d - v2)
                if not sdf >= -trunc:
                    continue
                m = sdf if sdf < trunc else trunc
                vol[i, j, k, 0] += int(np.rint(f32(m * scale)))
                vol[i, j, k, 1] += 1
    return vol


def _usable_scalar(S, W, min_weight):
    return W >= min_weight and abs(S) < QUANT * W


def extract_scalar(vol, lo, voxel, min_weight):
    lo, voxel = np.asarray(lo, f32).reshape(3), f32(voxel)
    dims = vol.shape[:3]
    out = []
    for i in range(dims[0]):
        for j in range(dims[1]):
            for k in range(dims[2]):
                S0, W0 = int(vol[i, j, k, 0]), int(vol[i, j, k, 1])
                if not _usable_scalar(S0, W0, min_weight):
                    continue
                ijk = (i, j, k)
                for a in range(3):
                    if ijk[a] + 1 >= dims[a]:
                        continue
                    nb = tuple(ijk[b] + (1 if b == a else 0) for b in range(3))
                    S1, W1 = int(vol[nb][0]), int(vol[nb][1])
                    if not _usable_scalar(S1, W1, min_weight) or (S0 < 0) == (S1 < 0):
                        continue
                    D0, D1 = f32(S0) / f32(W0), f32(S1) / f32(W1)
                    t = f32(D0 / f32(D0 - D1))
                    p = [lo[b] + f32((f32(ijk[b]) + f32(0.5)) * voxel) for b in range(3)]
                    p[a] = f32(p[a] + f32(t * voxel))
                    out.append(p)
    return np.asarray(out, f32).reshape(-1, 3)


def stats_scalar(vol, min_weight):
    observed = usable = 0
    for S, W in vol.reshape(-1, 2).tolist():
        observed += W > 0
        usable += _usable_scalar(S, W, min_weight)
    return {"observed_voxels": observed, "usable_voxels": usable}


# ---- what travels between ranks, and the record
def pack_raw(recon_raw, observed_voxels, usable_voxels, frames):
    """recon_metrics.pack_raw's float64 vector of the fused cloud, then observed_voxels, usable_voxels, frames (counts below 2^53
    are exact)."""
    return np.concatenate([np.asarray(recon_raw, np.float64).reshape(-1), np.array([observed_voxels, usable_voxels, frames], np.float64)])


def summarise_raw(raw, thresholds, cap, options=None):
    """A raw row -> the record's "fusion" block, JSON-safe: recon_metrics.summarise_raw's dict of the fused cloud (its n_points is
    the number of fused points) with observed_voxels, usable_voxels, frames and the options."""
    raw = np.asarray(raw, np.float64).reshape(-1)
    n = len(RAW_TAIL)
    out = recon_metrics.summarise_raw(raw[:-n], thresholds, cap)
    out.update({k: int(v) for k, v in zip(RAW_TAIL, raw[-n:])})
    if options is not None:
        out["options"] = dict(options)
    return out
