"""Shared inputs of the fused-mesh tests (tests/test_tsdf_mesh_host.py, tests/test_gpu_tsdf_mesh.py): volumes integrated from random
frames the way tests/test_gpu_tsdf.py builds them, the plane and the sphere with known answers, and a small GT box mesh with its
surface sample.  Each is computed once per process and handed out read-only."""
import functools

import numpy as np

from nextbestpath_amd.utility import tsdf, tsdf_mesh

f32 = np.float32
VOXEL, TRUNC, MAX_DEPTH, FAR = 0.3, 0.75, 9.0, 12.0
# (33, 9, 65): 19 305 voxels, 10 runs of 2048, no dimension a multiple of a wave or a workgroup: cells straddle every run boundary
DIMS = [(1, 1, 1), (1, 5, 7), (2, 2, 2), (3, 3, 3), (3, 5, 7), (33, 9, 65)]
MIN_WEIGHTS = (1, 2)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
H, W = 64, 114


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def geometry(dims):
    """The volume in front of the identity camera: its near face at z = 2."""
    return np.array([-0.5 * dims[0] * VOXEL + 0.1, -0.5 * dims[1] * VOXEL - 0.07, 2.0], f32)


def _lattice_cam(position, azim):
    from nextbestpath_amd.simulator.camera import Camera
    return Camera.cam12_of_pose(None, np.array([*position, 0.0, azim], f32))


def _cameras(dims):
    """The identity camera, and two lattice poses outside the volume looking at its centre along azimuths 45 and 315 degrees."""
    c = geometry(dims).astype(np.float64) + 0.5 * VOXEL * np.array(dims)
    out = [IDENTITY]
    for azim in (45.0, 315.0):
        a = np.deg2rad(azim)
        out.append(_lattice_cam(c - 6.0 * np.array([np.sin(a), 0.0, np.cos(a)]) + np.array([0.0, 0.4, 0.0]), azim))
    return np.stack(out).astype(f32)


def _frames(n, dims, seed):
    """Smooth random depth images whose surfaces pass through the volume (a tilted plane with a few low-frequency waves per frame,
    so that neighbouring voxels agree and the crossings form sheets), with 10 % invalid pixels: voxels seen by one, two or three
    frames, and voxels that only ever saw a far background (saturated)."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    depth = dims[2] * VOXEL
    out = []
    for f in range(n):
        base = (2.0 if f == 0 else 6.0 - 0.5 * depth) + depth * rng.uniform(0.3, 0.7)
        z = base + 0.35 * depth * (rng.uniform(-1, 1) * r + rng.uniform(-1, 1) * c) + 0.2 * depth * np.sin(3 * r + 5 * c + f)
        z = z.astype(f32)
        far = rng.random((H, W)) < 0.15
        z[far] = f32(FAR - 3.5)                                   # beyond the volume, within max_depth: saturates what it sees
        z[rng.random((H, W)) < 0.10] = -1.0
        out.append(z)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def random_volume(dims):
    """(vol int32 [nx,ny,nz,2] read-only, lo): three frames integrated by the definition."""
    lo = geometry(dims)
    vol = tsdf.empty_volume(dims)
    for z, cam in zip(_frames(3, dims, seed=dims[0] * 1000 + dims[2]), _cameras(dims)):
        tsdf.integrate(vol, lo, VOXEL, z, cam, TRUNC, MAX_DEPTH)
    vol.setflags(write=False)
    lo.setflags(write=False)
    return vol, lo


@functools.lru_cache(maxsize=None)
def random_mesh(dims, min_weight):
    vol, lo = random_volume(dims)
    return tsdf_mesh.mesh(vol, lo, VOXEL, min_weight)


# ---- the plane: W = 1, S = 4 i + 2 j + 8 k - 101 (odd: S is never 0)
# (16, 16, 12): S runs from -101 to 77, every voxel usable (|S| < 127), and the plane cuts the volume through its middle
PLANE_DIMS, PLANE_LO, PLANE_VOXEL = (16, 16, 12), np.array([-1.0, 0.5, 2.0], f32), 0.25


def plane_volume():
    i, j, k = np.meshgrid(*[np.arange(d) for d in PLANE_DIMS], indexing="ij")
    vol = np.stack([4 * i + 2 * j + 8 * k - 101, np.ones_like(i)], -1).astype(np.int32)
    return np.ascontiguousarray(vol), PLANE_LO


# ---- the sphere: 24^3 voxels of 0.25, trunc 1.0, S = rint(clip(|c - centre| - 2.1, +-trunc) 127), S == 0 -> 1, W = 1
SPHERE_DIMS, SPHERE_VOXEL, SPHERE_TRUNC, SPHERE_R = (24, 24, 24), 0.25, 1.0, 2.1
SPHERE_CENTRE, SPHERE_LO = np.array([0.02, -0.05, 0.01]), np.array([-3.03, -2.97, -3.01], f32)


@functools.lru_cache(maxsize=None)
def sphere_volume():
    c = tsdf.voxel_centres(SPHERE_LO, SPHERE_VOXEL, SPHERE_DIMS).astype(np.float64)
    d = np.sqrt(((c - SPHERE_CENTRE) ** 2).sum(1)) - SPHERE_R
    S = np.rint(np.clip(d, -SPHERE_TRUNC, SPHERE_TRUNC) * 127).astype(np.int32)
    S[S == 0] = 1
    vol = np.ascontiguousarray(np.stack([S, np.ones_like(S)], -1).reshape(*SPHERE_DIMS, 2))
    vol.setflags(write=False)
    return vol, SPHERE_LO


# ---- a GT for the metrics: an axis-aligned box mesh (12 triangles) and a sample of its surface
def gt_box(lo, hi, n, seed=0):
    """-> (verts float32 [8,3], faces int32 [12,3], sample float32 [n,3] on the faces)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts = np.array([[(lo, hi)[(m >> d) & 1][d] for d in range(3)] for m in range(8)], f32)
    faces = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                      [1, 3, 5], [3, 7, 5]], np.int32)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 12, n)
    u, v = rng.random(n), rng.random(n)
    swap = u + v > 1
    u[swap], v[swap] = 1 - u[swap], 1 - v[swap]
    a, b, c = (verts[faces[f, k]].astype(np.float64) for k in range(3))
    return verts, faces, (a + u[:, None] * (b - a) + v[:, None] * (c - a)).astype(f32)
