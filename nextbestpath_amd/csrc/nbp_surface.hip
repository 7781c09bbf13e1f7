// nbp_surface.hip -- accuracy of a cloud against the GT MESH: exact truncated point-to-triangle squared distances through a uniform
// grid of triangles (include/nbp_hip.h: nbp_mesh_*; the definition of record is nextbestpath_amd/utility/surface_metrics.py, which
// these kernels equal bit for bit).  Not in the reference.  The summary of the distances is nbp_recon.hip's
// nbp_recon_stats_f64 as it stands.
//
// Plan.  A triangle takes part iff its three indices are in range and its three vertices lie inside the caller's box (lo <= v <= hi
// in fp32; a NaN or an infinity is outside).  It is registered in every cell of the range spanned by the cells of its bounding box's
// two corners -- nbp_recon.hip's grid (nbp_nn_grid.h: cells 1.001 w wide) and grid_cell's fp32 expression, clamped.  The build is
// count (one atomicAdd per (triangle, cell)), grid_exclusive_scan, fill (a second atomicAdd per pair hands out the slot).  The
// number of pairs is known on the device only: the count call leaves it in device memory, the caller reads it back ONCE, at plan
// construction, allocates the entry list and calls fill, which writes nothing at or beyond the capacity it is given.  A triangle
// that covers more than MESH_SMALL cells is registered by the 64 lanes of its wave together (one floor-sized triangle would
// otherwise be tens of thousands of dependent atomics in one thread).  An entry is the triangle's index; the plan keeps the
// vertices of every participating triangle as three float4 (a, b, c, copied as they are: the kernel's b - a has the definition's
// bits).  The slot order inside a cell does not show: the result is a minimum.
//
// Query.  One launch: nbp_shell_walk.h's walk over the shells of cells around the query's UNCLAMPED cell, MESH_LANES lanes per query
// (a query beyond reach, or with a NaN, gets cap2 without a memory access; rows at or beyond the device counter are never read or
// written), point_triangle_d2 evaluated for every entry of every cell it visits.
//
// Why the walk's early exits hold for triangles.  point_triangle_d2 is the MAXIMUM of the core term (segments and face) and the box
// term, the fp32 squared distance from the query to the triangle's fp32 bounding box.  A triangle is registered in every cell of
// its range, and shells 0..r are every cell within r of the query's cell, so a triangle that shells 0..r have not shown has a cell
// range that misses [c - r, c + r] on some axis: its nearest cell there, which is the cell of the nearer face of its box (grid_cell
// is monotone), differs from the query's cell by at least r + 1.  That is the situation of nbp_shell_walk.h's proof with "target"
// read as "nearest point of the box": the box term's e on that axis, fl(lo - p) or fl(p - hi), has fl(e e) > fl(r w)^2, and --
// rounding being monotone and the other two squares non-negative -- so has the box term, and with it the maximum: the skipped
// triangle's point_triangle_d2 exceeds fl(r w)^2 >= best and cannot lower the minimum.  No bound on the size of a triangle or on
// the rounding error of the core term enters: that is what the box term is in the definition for.  So the result is the
// brute-force minimum over all participating triangles, bit for bit.  A triangle that spans several cells is evaluated more than
// once: that costs time, not bits.
#include "nbp_shell_walk.h"

#pragma clang fp contract(off)

namespace {

constexpr int MESH_LANES = 8;                    // lanes per query: the 8 rim columns of shell 1 at once
constexpr int MESH_UNROLL = 2;                   // triangles of a run in flight together (an entry is an index and three float4)
constexpr int MESH_SMALL = 32;                   // cells up to which a triangle's owner thread registers it alone
constexpr float MESH_GUARD = 5.9604644775390625e-08f;   // 2^-24: utility/surface_metrics.py GUARD

// ---- the definition, transcribed (utility/surface_metrics.py: min(x, y) is `y < x ? y : x`, max(x, y) is `y > x ? y : x`)
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ float seg_d2(float upx, float upy, float upz, float uvx, float uvy, float uvz) {
    const float den = dot3(uvx, uvy, uvz, uvx, uvy, uvz), num = dot3(upx, upy, upz, uvx, uvy, uvz);
    float t = den > 0.f ? num / den : 0.f;
    t = 0.f > t ? 0.f : t;
    t = 1.f < t ? 1.f : t;
    const float ex = upx - t * uvx, ey = upy - t * uvy, ez = upz - t * uvz;
    return dot3(ex, ey, ez, ex, ey, ez);
}

__device__ __forceinline__ float box_axis(float p, float a, float b, float c) {
    float lo = b < a ? b : a, hi = b > a ? b : a;
    lo = c < lo ? c : lo;
    hi = c > hi ? c : hi;
    float m = lo - p;
    const float m2 = p - hi;
    m = m2 > m ? m2 : m;
    return 0.f > m ? 0.f : m;
}

__device__ __forceinline__ float tri_d2(float px, float py, float pz, const float4 a, const float4 b, const float4 c) {
    const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z, apx = px - a.x, apy = py - a.y, apz = pz - a.z;
    const float bcx = c.x - b.x, bcy = c.y - b.y, bcz = c.z - b.z, bpx = px - b.x, bpy = py - b.y, bpz = pz - b.z;
    const float cax = a.x - c.x, cay = a.y - c.y, caz = a.z - c.z, cpx = px - c.x, cpy = py - c.y, cpz = pz - c.z;
    float core = seg_d2(apx, apy, apz, abx, aby, abz);
    float s = seg_d2(bpx, bpy, bpz, bcx, bcy, bcz);
    core = s < core ? s : core;
    s = seg_d2(cpx, cpy, cpz, cax, cay, caz);
    core = s < core ? s : core;
    const float acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float nn = dot3(nx, ny, nz, nx, ny, nz);
    bool ok = nn > MESH_GUARD * (dot3(abx, aby, abz, abx, aby, abz) * dot3(acx, acy, acz, acx, acy, acz));
    ok = ok && dot3(nx, ny, nz, aby * apz - abz * apy, abz * apx - abx * apz, abx * apy - aby * apx) >= 0.f;
    ok = ok && dot3(nx, ny, nz, bcy * bpz - bcz * bpy, bcz * bpx - bcx * bpz, bcx * bpy - bcy * bpx) >= 0.f;
    ok = ok && dot3(nx, ny, nz, cay * cpz - caz * cpy, caz * cpx - cax * cpz, cax * cpy - cay * cpx) >= 0.f;
    if (ok) {
        const float h = dot3(apx, apy, apz, nx, ny, nz);
        const float face = (h * h) / nn;
        core = face < core ? face : core;
    }
    const float ex = box_axis(px, a.x, b.x, c.x), ey = box_axis(py, a.y, b.y, c.y), ez = box_axis(pz, a.z, b.z, c.z);
    const float box = (ex * ex + ey * ey) + ez * ez;
    return box > core ? box : core;
}

// ---- plan
struct MeshRange { int c0[3], c1[3]; };

// Does triangle f take part?  Then its vertices and the inclusive range of cells it is registered in.
__device__ __forceinline__ bool mesh_triangle(const float* __restrict__ v, long long V, const int* __restrict__ faces, long long f,
                                              const Grid& g, const Box& bx, float4* a, float4* b, float4* c, MeshRange* r) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    *a = make_float4(v[3 * (size_t)i0], v[3 * (size_t)i0 + 1], v[3 * (size_t)i0 + 2], 0.f);
    *b = make_float4(v[3 * (size_t)i1], v[3 * (size_t)i1 + 1], v[3 * (size_t)i1 + 2], 0.f);
    *c = make_float4(v[3 * (size_t)i2], v[3 * (size_t)i2 + 1], v[3 * (size_t)i2 + 2], 0.f);
    if (!in_box(g, bx, a->x, a->y, a->z) || !in_box(g, bx, b->x, b->y, b->z) || !in_box(g, bx, c->x, c->y, c->z)) return false;
    grid_cell(g, fminf(fminf(a->x, b->x), c->x), fminf(fminf(a->y, b->y), c->y), fminf(fminf(a->z, b->z), c->z), r->c0);
    grid_cell(g, fmaxf(fmaxf(a->x, b->x), c->x), fmaxf(fmaxf(a->y, b->y), c->y), fmaxf(fmaxf(a->z, b->z), c->z), r->c1);
    return true;
}

// Calls fn(cell, f) for every cell of every lane's triangle (ok: the lane has one).  Reached by all 64 lanes of the wave: a range of
// more than MESH_SMALL cells is walked by the whole wave, lane by lane of its owners.
template <class Fn>
__device__ __forceinline__ void mesh_for_cells(const Grid& g, bool ok, const MeshRange& r, int f, Fn fn) {
    const int d1 = r.c1[1] - r.c0[1] + 1, d2 = r.c1[2] - r.c0[2] + 1;
    const int n = ok ? (r.c1[0] - r.c0[0] + 1) * d1 * d2 : 0;        // <= the grid's 2^28 cells
    if (n <= MESH_SMALL)
        for (int i = r.c0[0]; ok && i <= r.c1[0]; ++i)
            for (int j = r.c0[1]; j <= r.c1[1]; ++j)
                for (int k = r.c0[2]; k <= r.c1[2]; ++k) fn((i * g.n[1] + j) * g.n[2] + k, f);
    const int lane = threadIdx.x & 63;
    for (unsigned long long big = __ballot(n > MESH_SMALL); big; big &= big - 1) {
        const int src = __ffsll((long long)big) - 1;
        const int bi = __shfl(r.c0[0], src), bj = __shfl(r.c0[1], src), bk = __shfl(r.c0[2], src);
        const int e1 = __shfl(d1, src), e2 = __shfl(d2, src), bn = __shfl(n, src), bf = __shfl(f, src);
        for (int t = lane; t < bn; t += 64) {
            const int i = bi + t / (e1 * e2), j = bj + t / e2 % e1, k = bk + t % e2;
            fn((i * g.n[1] + j) * g.n[2] + k, bf);
        }
    }
}

// totals[0] += the (triangle, cell) pairs, totals[1] += the participating triangles; tri [3 F] gets their vertices
__global__ __launch_bounds__(256) void mesh_count_kernel(const float* __restrict__ v, long long V, const int* __restrict__ faces,
                                                         long long F, Grid g, Box bx, float4* __restrict__ tri,
                                                         int* __restrict__ count, unsigned long long* __restrict__ totals) {
    long long pairs = 0, used = 0;
    // (base is the same in the 64 lanes of a wave: all of them reach mesh_for_cells)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < F; base += (long long)gridDim.x * blockDim.x) {
        const long long f = base + threadIdx.x;
        float4 a, b, c;
        MeshRange r = {{0, 0, 0}, {0, 0, 0}};
        const bool ok = f < F && mesh_triangle(v, V, faces, f, g, bx, &a, &b, &c, &r);
        if (ok) {
            tri[3 * f] = a; tri[3 * f + 1] = b; tri[3 * f + 2] = c;
            pairs += (long long)(r.c1[0] - r.c0[0] + 1) * (r.c1[1] - r.c0[1] + 1) * (r.c1[2] - r.c0[2] + 1);
            used += 1;
        }
        mesh_for_cells(g, ok, r, (int)f, [&](int cell, int) { atomicAdd(&count[cell], 1); });
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pairs += __shfl_down(pairs, off, 64);
        used += __shfl_down(used, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && used) {
        atomicAdd(&totals[0], (unsigned long long)pairs);
        atomicAdd(&totals[1], (unsigned long long)used);
    }
}

__global__ __launch_bounds__(256) void mesh_fill_kernel(const float* __restrict__ v, long long V, const int* __restrict__ faces,
                                                        long long F, Grid g, Box bx, const int* __restrict__ start,
                                                        int* __restrict__ cursor, int* __restrict__ entries, long long capacity) {
    for (long long base = (long long)blockIdx.x * blockDim.x; base < F; base += (long long)gridDim.x * blockDim.x) {
        const long long f = base + threadIdx.x;
        float4 a, b, c;
        MeshRange r = {{0, 0, 0}, {0, 0, 0}};
        const bool ok = f < F && mesh_triangle(v, V, faces, f, g, bx, &a, &b, &c, &r);
        mesh_for_cells(g, ok, r, (int)f, [&](int cell, int owner) {
            const long long at = (long long)start[cell] + atomicAdd(&cursor[cell], 1);
            if (at >= 0 && at < capacity) entries[at] = owner;       // nothing at or beyond the caller's capacity
        });
    }
}

// ---- query: the shell walk over cells of triangle entries
__device__ __forceinline__ float mesh_run(const int* __restrict__ entries, const float4* __restrict__ tri, int p, int hi, float x,
                                          float y, float z, float best) {
    for (; p + MESH_UNROLL <= hi; p += MESH_UNROLL) {
        float4 t[MESH_UNROLL][3];
#pragma unroll
        for (int u = 0; u < MESH_UNROLL; ++u) {
            const size_t f = (size_t)entries[p + u];
            t[u][0] = tri[3 * f]; t[u][1] = tri[3 * f + 1]; t[u][2] = tri[3 * f + 2];
        }
#pragma unroll
        for (int u = 0; u < MESH_UNROLL; ++u) {
            const float d = tri_d2(x, y, z, t[u][0], t[u][1], t[u][2]);
            best = d < best ? d : best;
        }
    }
    for (; p < hi; ++p) {
        const size_t f = (size_t)entries[p];
        const float d = tri_d2(x, y, z, tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]);
        best = d < best ? d : best;
    }
    return best;
}

struct MeshTriangles {
    static constexpr int LANES = MESH_LANES;
    const int* __restrict__ entries;
    const float4* __restrict__ tri;
    __device__ __forceinline__ float run(int p, int hi, float x, float y, float z, float best) const {
        return mesh_run(entries, tri, p, hi, x, y, z, best);
    }
};

// ---- host
// a plan holds max(F, 1) triangles, three float4 vertices each
size_t mesh_plan_bytes(size_t ncell, long long F) { return carved_bytes(0, nn_plan_layout, ncell, (size_t)(F > 0 ? F : 1) * 3); }

}  // namespace

extern "C" size_t nbp_mesh_plan_bytes(const float* lo_host, const float* hi_host, float cell, long long F) {
    BoxGrid b;
    return nn_count_ok(F) && !nn_grid(lo_host, hi_host, cell, &b) ? mesh_plan_bytes(b.ncell, F) : 0;
}

extern "C" size_t nbp_mesh_plan_workspace_bytes(const float* lo_host, const float* hi_host, float cell) {
    BoxGrid b;
    return nn_grid(lo_host, hi_host, cell, &b) ? 0 : nn_scratch_bytes(b.ncell);
}

extern "C" int nbp_mesh_plan_count_f32(const float* verts3, long long V, const int* faces3, long long F, const float* lo_host,
                                       const float* hi_host, float cell, void* plan, size_t plan_bytes, long long* totals2_dev,
                                       void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!plan || !ws || !totals2_dev || !nn_args_ok(lo_host, hi_host, cell) || !nn_count_ok(V) || !nn_count_ok(F), NBP_E_ARG);
    NBP_RETURN_IF(F > 0 && (!faces3 || (V > 0 && !verts3)), NBP_E_ARG);
    NBP_RETURN_IF(((uintptr_t)totals2_dev & 7), NBP_E_SHAPE);
    BoxGrid b;
    int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    NBP_RETURN_IF(plan_bytes < mesh_plan_bytes(b.ncell, F) || ws_bytes < nn_scratch_bytes(b.ncell), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    const NNPlan pl = nn_plan_of(plan, b.ncell);
    const NNScratch w = carve(ws, nn_scratch_layout, b.ncell);
    hipError_t e = hipMemsetAsync(w.count, 0, b.ncell * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(totals2_dev, 0, 16, st);
    if (e != hipSuccess) return (int)e;
    if (F > 0) {
        mesh_count_kernel<<<nbp_ew_grid(F, 256), 256, 0, st>>>(verts3, V, faces3, F, b.g, b.bx, pl.payload, w.count,
                                                                 (unsigned long long*)totals2_dev);
        if ((rc = nbp_launch_status())) return rc;
    }
    return grid_exclusive_scan(w.count, (long long)b.ncell, w.tsum, pl.start, st);
}

extern "C" int nbp_mesh_plan_fill_i32(const float* verts3, long long V, const int* faces3, long long F, const float* lo_host,
                                      const float* hi_host, float cell, const void* plan, int* entries, long long entry_capacity,
                                      void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!plan || !ws || !nn_args_ok(lo_host, hi_host, cell) || !nn_count_ok(V) || !nn_count_ok(F) || entry_capacity < 0,
                  NBP_E_ARG);
    NBP_RETURN_IF((F > 0 && (!faces3 || (V > 0 && !verts3))) || (entry_capacity > 0 && !entries), NBP_E_ARG);
    NBP_RETURN_IF(entry_capacity > 0x7fffffffll, NBP_E_SHAPE);         // an entry's position is an int of the scan
    BoxGrid b;
    const int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    NBP_RETURN_IF(ws_bytes < nn_scratch_bytes(b.ncell), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    const NNPlan pl = nn_plan_of(plan, b.ncell);
    int* cursor = carve(ws, nn_scratch_layout, b.ncell).count;
    hipError_t e = hipMemsetAsync(cursor, 0, b.ncell * 4, st);
    if (e != hipSuccess) return (int)e;
    if (F == 0) return 0;
    mesh_fill_kernel<<<nbp_ew_grid(F, 256), 256, 0, st>>>(verts3, V, faces3, F, b.g, b.bx, pl.start, cursor, entries, entry_capacity);
    return nbp_launch_status();
}

extern "C" int nbp_mesh_dist2_planned_f32(const void* plan, const int* entries, const float* lo_host, const float* hi_host, float cell,
                                          float cap, const float* q3, long long Q, const long long* Q_dev_or_null, float* d2,
                                          void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!plan || !entries || !nn_args_ok(lo_host, hi_host, cell) || !nn_cap_ok(cap, cell) || !nn_count_ok(Q), NBP_E_ARG);
    NBP_RETURN_IF(Q > 0 && (!q3 || !d2), NBP_E_ARG);
    BoxGrid b;
    const int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    const NNPlan pl = nn_plan_of(plan, b.ncell);
    return shell_query(MeshTriangles{entries, pl.payload}, pl.start, b.g, cap, cell, q3, Q, Q_dev_or_null, d2, (hipStream_t)stream);
}
