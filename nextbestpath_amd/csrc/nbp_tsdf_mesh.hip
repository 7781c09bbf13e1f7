// nbp_tsdf_mesh.hip -- a triangle mesh out of the TSDF volume by naive surface nets (include/nbp_hip.h: nbp_tsdf_mesh_*; the
// definition, which this file equals bit for bit, is nextbestpath_amd/utility/tsdf_mesh.py).  Not in the reference.
//
// One vertex per grid cell that holds a crossing of nbp_tsdf.hip's extraction (the mean of the cell's crossing points, added in
// edge order), one quad = two triangles per crossing whose four surrounding cells exist.  Vertices come in cell order, faces in the
// extraction's order (voxel, axis), so that what reads them reduces in a fixed order: fp32 with one rounding per operation (no
// contraction in this file), no atomics.
//
// Passes, in the extraction's shape.  A cell has the linear index of its low corner voxel, so cells and crossings share ONE
// partition into runs of EX_RUN consecutive voxels, a workgroup each:
//   count   per run, its active cells and its emitting crossings;
//   scan    one workgroup: both count arrays -> exclusive offsets, the totals (vertices, faces = 2 quads) into device memory.
//           With both capacities 0 the call ends here;
//   verts   recomputes each active cell's vertex, writes it at run offset + prefix inside the workgroup (rows below the capacity
//           only), and writes that id into a dense int32 [n_voxels] map in the workspace.  The map is not cleared: the face pass
//           reads only cells that contain a crossing, and those were all written by this launch;
//   faces   recomputes each voxel's crossings, looks the four ids up and writes the two triangles (rows below the capacity only;
//           an id at or beyond the VERTEX capacity is still written: ids are ranks, not addresses).  Where area2 is wanted, a vertex
//           below the vertex capacity is read back from the caller's buffer and one beyond it -- the buffer may be short or absent
//           -- is made again from the volume, by the same operations.
//
// Corners: global loads, no LDS brick.  A cell reads its eight corners (S, W) straight from the volume; a voxel is read by the
// eight cells around it.  Lanes run along k, so the two k-corners of a wave are one 520-byte stretch and a cell's eight loads fall
// on four such stretches (j, j + 1 of planes i, i + 1); the re-reads by the neighbouring rows and planes come a few workgroups
// later, out of L2 or the last-level cache, where DESIGN.md 4q measured a 33 MB volume to stay resident.  A brick in LDS would
// save those cache hits at the price of a halo per run -- runs are stretches of the LINEAR index, not bricks, because the output
// order is linear -- and of a second partition beside the extraction's.  Not measured against each other: DESIGN.md 4s has what
// was measured.
#include "nbp_tsdf_shared.h"

#pragma clang fp contract(off)

namespace {

// corner m = 4 di + 2 dj + dk of a cell; edge e = 4 a + 2 beta + gamma runs from corner EDGE_LO[e] one step up axis a
__device__ constexpr int EDGE_LO[12] = {0, 1, 2, 3, 0, 1, 4, 5, 0, 2, 4, 6};
__device__ constexpr int EDGE_STEP[3] = {4, 2, 1};

struct Cell {
    int2 sw[8];
    unsigned edges;                                  // bit e: edge e is a crossing
};

// the cell with low corner (i, j, k) at linear index v; the caller guarantees that it exists
__device__ __forceinline__ void load_cell(const int2* __restrict__ vol, const ExGeom& g, long long v, Cell& c) {
    const long long si = (long long)g.ny * g.nz, sj = g.nz;
    unsigned use = 0, neg = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int2 s = vol[v + (m & 4 ? si : 0) + (m & 2 ? sj : 0) + (m & 1)];
        c.sw[m] = s;
        use |= tsdf_usable(s, g.min_weight) ? 1u << m : 0u;
        neg |= s.x < 0 ? 1u << m : 0u;
    }
    unsigned edges = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int m0 = EDGE_LO[e], m1 = m0 + EDGE_STEP[e >> 2];
        const bool both = ((use >> m0) & (use >> m1) & 1u) != 0, differ = (((neg >> m0) ^ (neg >> m1)) & 1u) != 0;
        edges |= both && differ ? 1u << e : 0u;
    }
    c.edges = edges;
}

// voxel v -> (i, j, k); whether it is a cell's low corner
__device__ __forceinline__ bool voxel_cell(const ExGeom& g, long long v, long long n_vox, int* ijk) {
    if (v >= n_vox) return false;
    const long long ij = v / g.nz;
    ijk[2] = (int)(v % g.nz);
    ijk[1] = (int)(ij % g.ny);
    ijk[0] = (int)(ij / g.ny);
    return ijk[0] + 1 < g.nx && ijk[1] + 1 < g.ny && ijk[2] + 1 < g.nz;
}

// bit a: the crossing (v, a) -- the cell's edge 4 a, which starts at its low corner -- emits a quad: it exists and
// 1 <= v[b], v[c] <= dims - 2 on the other two axes
__device__ __forceinline__ unsigned emitting(const ExGeom& g, const int* ijk, unsigned edges) {
    const bool in0 = ijk[0] >= 1, in1 = ijk[1] >= 1, in2 = ijk[2] >= 1;      // (the upper bounds: the cell exists)
    unsigned q = 0;
    q |= (edges & (1u << 0)) && in1 && in2 ? 1u : 0u;
    q |= (edges & (1u << 4)) && in2 && in0 ? 2u : 0u;
    q |= (edges & (1u << 8)) && in0 && in1 ? 4u : 0u;
    return q;
}

// the vertex of an active cell: +0, plus its crossing points in edge order, over their number
__device__ __forceinline__ void cell_vertex(const ExGeom& g, const int* ijk, const Cell& c, float* out) {
    float acc[3] = {0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!(c.edges & (1u << e))) continue;
        const int a = e >> 2, m0 = EDGE_LO[e], m1 = m0 + EDGE_STEP[a];
        const float D0 = (float)c.sw[m0].x / (float)c.sw[m0].y, D1 = (float)c.sw[m1].x / (float)c.sw[m1].y;
        const float t = D0 / (D0 - D1);
        const float step = t * g.voxel;
        const float p0 = tsdf_centre(g.lo[0], ijk[0] + ((m0 >> 2) & 1), g.voxel), p1 = tsdf_centre(g.lo[1], ijk[1] + ((m0 >> 1) & 1), g.voxel),
                    p2 = tsdf_centre(g.lo[2], ijk[2] + (m0 & 1), g.voxel);
        acc[0] = acc[0] + (a == 0 ? p0 + step : p0);
        acc[1] = acc[1] + (a == 1 ? p1 + step : p1);
        acc[2] = acc[2] + (a == 2 ? p2 + step : p2);
        ++cnt;
    }
    const float n = (float)cnt;
    out[0] = acc[0] / n;
    out[1] = acc[1] / n;
    out[2] = acc[2] / n;
}

// the vertex of the (active) cell at (i, j, k), from the volume
__device__ __noinline__ void vertex_at(const int2* __restrict__ vol, const ExGeom& g, int i, int j, int k, float* out) {
    const int ijk[3] = {i, j, k};
    Cell c;
    load_cell(vol, g, ((long long)i * g.ny + j) * g.nz + k, c);
    cell_vertex(g, ijk, c, out);
}

// surface_metrics' dot and cross: f32(0.25) dot(n, n), n = cross(v1 - v0, v2 - v0)
__device__ __forceinline__ float tri_area2(const float* v0, const float* v1, const float* v2) {
    const float u0 = v1[0] - v0[0], u1 = v1[1] - v0[1], u2 = v1[2] - v0[2];
    const float w0 = v2[0] - v0[0], w1 = v2[1] - v0[1], w2 = v2[2] - v0[2];
    const float n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    return 0.25f * ((n0 * n0 + n1 * n1) + n2 * n2);
}

__global__ __launch_bounds__(TS_THREADS) void mesh_count_kernel(const int2* __restrict__ vol, ExGeom g, long long n_vox,
                                                                long long* __restrict__ run_cells, long long* __restrict__ run_quads) {
    __shared__ int wave_sums[TS_THREADS / 64];
    int cells = 0, quads = 0;
    const long long base = (long long)blockIdx.x * EX_RUN;
    for (int r = 0; r < EX_RUN / TS_THREADS; ++r) {
        const long long v = base + r * TS_THREADS + threadIdx.x;
        int ijk[3];
        if (!voxel_cell(g, v, n_vox, ijk)) continue;
        Cell c;
        load_cell(vol, g, v, c);
        cells += c.edges ? 1 : 0;
        quads += __popc(emitting(g, ijk, c.edges));
    }
    int total_cells, total_quads;
    block_inclusive_scan(cells, wave_sums, &total_cells);
    block_inclusive_scan(quads, wave_sums, &total_quads);
    if (threadIdx.x == 0) {
        run_cells[blockIdx.x] = total_cells;
        run_quads[blockIdx.x] = total_quads;
    }
}

// one workgroup: both count arrays -> exclusive offsets, in place; totals2 = (vertices, faces)
__global__ __launch_bounds__(TS_THREADS) void mesh_scan_kernel(long long* __restrict__ run_cells, long long* __restrict__ run_quads,
                                                               long long n_runs, long long* __restrict__ totals2) {
    __shared__ long long wave_sums[TS_THREADS / 64];
    const long long cells = scan_runs(run_cells, n_runs, wave_sums);
    const long long quads = scan_runs(run_quads, n_runs, wave_sums);
    if (threadIdx.x == 0) {
        totals2[0] = cells;
        totals2[1] = 2 * quads;
    }
}

__global__ __launch_bounds__(TS_THREADS) void mesh_verts_kernel(const int2* __restrict__ vol, ExGeom g, long long n_vox,
                                                                const long long* __restrict__ run_cells, float* __restrict__ verts,
                                                                long long capacity, int* __restrict__ vertex_of) {
    __shared__ int wave_sums[TS_THREADS / 64];
    long long at = run_cells[blockIdx.x];
    const long long base = (long long)blockIdx.x * EX_RUN;
    for (int r = 0; r < EX_RUN / TS_THREADS; ++r) {
        const long long v = base + r * TS_THREADS + threadIdx.x;
        int ijk[3] = {0, 0, 0};
        Cell c;
        c.edges = 0;
        if (voxel_cell(g, v, n_vox, ijk)) load_cell(vol, g, v, c);
        const int active = c.edges ? 1 : 0;
        int total;
        const int incl = block_inclusive_scan(active, wave_sums, &total);
        if (active) {
            const long long id = at + incl - 1;
            vertex_of[v] = (int)id;
            if (id < capacity) {
                float p[3];
                cell_vertex(g, ijk, c, p);
                verts[3 * id] = p[0];
                verts[3 * id + 1] = p[1];
                verts[3 * id + 2] = p[2];
            }
        }
        at += total;
    }
}

__global__ __launch_bounds__(TS_THREADS) void mesh_faces_kernel(const int2* __restrict__ vol, ExGeom g, long long n_vox,
                                                                const long long* __restrict__ run_quads,
                                                                const int* __restrict__ vertex_of, const float* __restrict__ verts,
                                                                long long vert_capacity, int* __restrict__ faces,
                                                                float* __restrict__ area2, long long capacity) {
    __shared__ int wave_sums[TS_THREADS / 64];
    long long at = run_quads[blockIdx.x];
    const long long base = (long long)blockIdx.x * EX_RUN;
    const long long stride[3] = {(long long)g.ny * g.nz, g.nz, 1};
    for (int r = 0; r < EX_RUN / TS_THREADS; ++r) {
        const long long v = base + r * TS_THREADS + threadIdx.x;
        int ijk[3] = {0, 0, 0};
        Cell c;
        c.edges = 0;
        c.sw[0] = {0, 1};
        if (voxel_cell(g, v, n_vox, ijk)) load_cell(vol, g, v, c);
        const unsigned q = emitting(g, ijk, c.edges);
        const int cnt = __popc(q);
        int total;
        const int incl = block_inclusive_scan(cnt, wave_sums, &total);
        long long quad = at + incl - cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(q & (1u << a))) continue;
            const int b = a == 2 ? 0 : a + 1, cc = b == 2 ? 0 : b + 1;      // the cyclic pair: the ring turns from b to c
            const bool keep = c.sw[0].x < 0;
            int id[4];
            int cell[4][3];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                // ring place s = the cell (-1,-1), (0,-1), (0,0), (-1,0) around the edge; S0 >= 0: the ring runs the other way round
                const int s = keep ? n : (4 - n) & 3;
                const int ob = s == 0 || s == 3 ? -1 : 0, oc = s < 2 ? -1 : 0;
                id[n] = vertex_of[v + ob * stride[b] + oc * stride[cc]];
                cell[n][0] = ijk[0];
                cell[n][1] = ijk[1];
                cell[n][2] = ijk[2];
                cell[n][b] += ob;
                cell[n][cc] += oc;
            }
            const long long row = 2 * quad;
            if (row < capacity) {
                faces[3 * row] = id[0];
                faces[3 * row + 1] = id[1];
                faces[3 * row + 2] = id[2];
            }
            if (row + 1 < capacity) {
                faces[3 * row + 3] = id[0];
                faces[3 * row + 4] = id[2];
                faces[3 * row + 5] = id[3];
            }
            if (area2 && row < capacity) {
                // a vertex the caller's buffer holds is read back; one beyond its capacity is made again from the volume: the
                // same operations in the same order, the same bits
                float p[4][3];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if (id[n] < vert_capacity) {
                        p[n][0] = verts[3 * (long long)id[n]];
                        p[n][1] = verts[3 * (long long)id[n] + 1];
                        p[n][2] = verts[3 * (long long)id[n] + 2];
                    } else {
                        vertex_at(vol, g, cell[n][0], cell[n][1], cell[n][2], p[n]);
                    }
                }
                area2[row] = tri_area2(p[0], p[1], p[2]);
                if (row + 1 < capacity) area2[row + 1] = tri_area2(p[0], p[2], p[3]);
            }
            ++quad;
        }
        at += total;
    }
}

struct Span { const void* p; size_t n; };

}  // namespace

extern "C" size_t nbp_tsdf_mesh_workspace_bytes(long long n_voxels) {
    if (n_voxels < 1 || n_voxels > TS_MAX_VOXELS) return 0;
    return 256 + (size_t)extract_runs(n_voxels) * 16 + (size_t)n_voxels * 4;
}

extern "C" int nbp_tsdf_mesh_f32(const int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, int min_weight,
                                 float* verts_or_null, long long vert_capacity, int* faces_or_null, float* area2_or_null,
                                 long long face_capacity, long long* totals2, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    int rc = check_geometry(vol, lo_host, voxel, nx, ny, nz);
    if (rc) return rc;
    NBP_RETURN_IF(!totals2 || !ws || min_weight < 1 || vert_capacity < 0 || face_capacity < 0 || (vert_capacity > 0 && !verts_or_null) ||
                      (face_capacity > 0 && !faces_or_null),
                  NBP_E_ARG);
    NBP_RETURN_IF(((uintptr_t)totals2 & 7), NBP_E_SHAPE);
    const long long n_vox = (long long)nx * ny * nz;
    NBP_RETURN_IF(ws_bytes < nbp_tsdf_mesh_workspace_bytes(n_vox), NBP_E_WS);
    const long long n_runs = extract_runs(n_vox);
    long long* run_cells = (long long*)(((uintptr_t)ws + 255) / 256 * 256);
    long long* run_quads = run_cells + n_runs;
    int* vertex_of = (int*)(run_quads + n_runs);
    // the volume, the totals, the workspace in use and the outputs that will be written: no two may overlap
    const Span spans[6] = {{vol, (size_t)n_vox * 8},
                           {totals2, 16},
                           {run_cells, (size_t)n_runs * 16 + (size_t)n_vox * 4},
                           {verts_or_null, vert_capacity > 0 ? (size_t)vert_capacity * 12 : 0},
                           {faces_or_null, face_capacity > 0 ? (size_t)face_capacity * 12 : 0},
                           {area2_or_null, face_capacity > 0 && area2_or_null ? (size_t)face_capacity * 4 : 0}};
    for (int x = 0; x < 6; ++x)
        for (int y = x + 1; y < 6; ++y)
            NBP_RETURN_IF(spans[x].n && spans[y].n && ranges_overlap(spans[x].p, spans[x].n, spans[y].p, spans[y].n), NBP_E_ARG);
    hipStream_t st = (hipStream_t)stream;
    ExGeom g = {{lo_host[0], lo_host[1], lo_host[2]}, voxel, nx, ny, nz, min_weight};
    mesh_count_kernel<<<(unsigned)n_runs, TS_THREADS, 0, st>>>((const int2*)vol, g, n_vox, run_cells, run_quads);
    rc = nbp_launch_status();
    if (rc) return rc;
    mesh_scan_kernel<<<1, TS_THREADS, 0, st>>>(run_cells, run_quads, n_runs, totals2);
    rc = nbp_launch_status();
    if (rc || (vert_capacity == 0 && face_capacity == 0)) return rc;
    mesh_verts_kernel<<<(unsigned)n_runs, TS_THREADS, 0, st>>>((const int2*)vol, g, n_vox, run_cells, verts_or_null, vert_capacity,
                                                               vertex_of);
    rc = nbp_launch_status();
    if (rc || face_capacity == 0) return rc;
    mesh_faces_kernel<<<(unsigned)n_runs, TS_THREADS, 0, st>>>((const int2*)vol, g, n_vox, run_quads, vertex_of, verts_or_null,
                                                               vert_capacity, faces_or_null, area2_or_null, face_capacity);
    return nbp_launch_status();
}
