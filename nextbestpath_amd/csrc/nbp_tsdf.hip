// nbp_tsdf.hip -- TSDF fusion of depth frames into an integer volume, and the fused surface cloud taken out of it
// (include/nbp_hip.h: nbp_tsdf_*; the definition, which this file equals bit for bit, is nextbestpath_amd/utility/tsdf.py;
// DESIGN.md 4q).  Not in the reference.
//
// Volume: int32 [nx][ny][nz][2], voxel (i, j, k) at linear index (i ny + j) nz + k holds (S, W) = (sum of quantised signed
// distances, number of observations).
//
// Integration.  A thread owns a voxel (lanes run along k, the contiguous axis: a wave reads and writes 512 consecutive bytes).  It
// loads (S, W) once with one 8-byte access, loops over the launch's <= 4 frames in registers and stores once, and only if some
// frame updated it: in a maze most voxels inside a frustum lie hidden behind a wall.  The projection is nbp_camera.h's `project`
// (view_metrics.project), fp32 with one rounding per operation (no contraction in this file).  The sums are integers and a voxel
// has one owner: no atomics, and frames integrated in any order or grouping give the same bits.  Pointers, geometry and cameras
// ride in the kernel arguments (12 items of 280 bytes in the batch form: under 4 KB); both launch forms run ONE device body.
// No brick cull: every voxel of the volume is projected into every frame (DESIGN.md 4q gives the cost).
//
// Extraction.  The point list comes in the definition's order (linear index, axis), so that what reads it reduces in a fixed order:
// a count launch (one workgroup per run of EX_RUN consecutive voxels), a one-workgroup exclusive scan of the runs' counts that also
// leaves the total in device memory, and an emit launch that recomputes each voxel's crossings and writes them at the run's offset
// plus a prefix sum inside the workgroup.  Rows at or beyond the caller's capacity are not written.
//
// Statistics.  Two integer counts through nbp_stat_rows.h's fixed-order fold (ST_BLOCKS blocks, a row being the two counts).
#include "nbp_tsdf_shared.h"
#include "nbp_camera.h"
#include "nbp_stat_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int TS_ITEMS = 12;                        // the step's group stages chunk at 12 items (nbp_sim.hip: STEP_BATCH) ...
constexpr int TS_FRAMES = 4;                        // ... of <= 4 frames each
constexpr long long TS_MAX_PIXELS = 1ll << 29;
constexpr int ST_BLOCKS = 256, ST_COUNTS = 2;
static_assert(TS_THREADS == STAT_THREADS, "the statistics run in the fold's block size");

// one volume with its geometry, its fusion constants and the frames of one launch: 280 bytes
struct TsdfItem {
    int2* vol;
    const float* frame[TS_FRAMES];
    float lo[3];
    float voxel;
    int nx, ny, nz;
    int n_frames;
    float trunc, scale, max_depth;
    int pad;
    Cam cam[TS_FRAMES];
};
struct TsdfBatch { TsdfItem it[TS_ITEMS]; };
static_assert(sizeof(TsdfItem) == 280, "TsdfItem is 280 bytes");
static_assert(sizeof(TsdfBatch) + 64 <= 4096, "the batch form's argument block stays under 4 KB");

// ONE body for both launch forms: voxel `v` of `it` (the item lives in the kernel arguments; its indices are uniform)
__device__ __forceinline__ void integrate_voxel(const TsdfItem& it, long long v, int H, int W, float tanh_fov, float z_clip) {
    const long long n_vox = (long long)it.nx * it.ny * it.nz;
    if (v >= n_vox) return;
    const int k = (int)(v % it.nz);
    const long long ij = v / it.nz;
    const int j = (int)(ij % it.ny), i = (int)(ij / it.ny);
    const float p[3] = {tsdf_centre(it.lo[0], i, it.voxel), tsdf_centre(it.lo[1], j, it.voxel), tsdf_centre(it.lo[2], k, it.voxel)};
    const NdcTables nt(H, W);
    const float row_hi = (float)(H - 1), col_hi = (float)(W - 1);
    const float z_far = __builtin_inff();
    const float trunc = it.trunc, scale = it.scale, max_depth = it.max_depth;
    int2 sw = it.vol[v];
    bool touched = false;
    for (int c = 0; c < it.n_frames; ++c) {
        float fr, fc, v2;
        if (!project(p, it.cam[c], nt, tanh_fov, z_clip, z_far, &fr, &fc, &v2)) continue;
        // outside the image (decided on the FLOATS: only an in-range value reaches the int conversion)
        if (!(fr >= 0.f && fr <= row_hi && fc >= 0.f && fc <= col_hi)) continue;
        const float d = it.frame[c][(size_t)(int)fr * W + (int)fc];
        if (!(d > -1.0f && d <= max_depth)) continue;                // (a NaN fails the first)
        const float sdf = d - v2;
        if (!(sdf >= -trunc)) continue;
        const float q = fminf(sdf, trunc) * scale;
        sw.x += (int)rintf(q);
        sw.y += 1;
        touched = true;
    }
    if (touched) it.vol[v] = sw;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(TsdfItem it, int H, int W, float tanh_fov, float z_clip) {
    integrate_voxel(it, (long long)blockIdx.x * TS_THREADS + threadIdx.x, H, W, tanh_fov, z_clip);
}

// item blockIdx.y of the batch (a workgroup beyond its item's voxels leaves at once)
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_batch_kernel(TsdfBatch b, int H, int W, float tanh_fov, float z_clip) {
    integrate_voxel(b.it[blockIdx.y], (long long)blockIdx.x * TS_THREADS + threadIdx.x, H, W, tanh_fov, z_clip);
}

// ---- extraction
// the crossings of voxel v: bit a = one point on axis a.  d0 / d1[a]: the voxel's and its neighbours' (S, W)
__device__ __forceinline__ int tsdf_crossings(const int2* __restrict__ vol, const ExGeom& g, long long v, long long n_vox, int* ijk,
                                              int2* own, int2* nb) {
    if (v >= n_vox) return 0;
    const int k = (int)(v % g.nz);
    const long long ij = v / g.nz;
    ijk[2] = k;
    ijk[1] = (int)(ij % g.ny);
    ijk[0] = (int)(ij / g.ny);
    const int2 s0 = vol[v];
    *own = s0;
    if (!tsdf_usable(s0, g.min_weight)) return 0;
    int m = 0;
    if (ijk[0] + 1 < g.nx) {
        const int2 s1 = vol[v + (long long)g.ny * g.nz];
        nb[0] = s1;
        if (tsdf_usable(s1, g.min_weight) && ((s0.x < 0) != (s1.x < 0))) m |= 1;
    }
    if (ijk[1] + 1 < g.ny) {
        const int2 s1 = vol[v + g.nz];
        nb[1] = s1;
        if (tsdf_usable(s1, g.min_weight) && ((s0.x < 0) != (s1.x < 0))) m |= 2;
    }
    if (ijk[2] + 1 < g.nz) {
        const int2 s1 = vol[v + 1];
        nb[2] = s1;
        if (tsdf_usable(s1, g.min_weight) && ((s0.x < 0) != (s1.x < 0))) m |= 4;
    }
    return m;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_count_kernel(const int2* __restrict__ vol, ExGeom g, long long n_vox,
                                                                long long* __restrict__ run_counts) {
    __shared__ int wave_sums[TS_THREADS / 64];
    int cnt = 0;
    const long long base = (long long)blockIdx.x * EX_RUN;
    for (int r = 0; r < EX_RUN / TS_THREADS; ++r) {
        int ijk[3];
        int2 own, nb[3];
        cnt += __popc(tsdf_crossings(vol, g, base + r * TS_THREADS + threadIdx.x, n_vox, ijk, &own, nb));
    }
    int total;
    block_inclusive_scan(cnt, wave_sums, &total);
    if (threadIdx.x == 0) run_counts[blockIdx.x] = total;
}

// one workgroup: run_counts -> exclusive offsets, in place; the total into total_dev
__global__ __launch_bounds__(TS_THREADS) void tsdf_scan_kernel(long long* __restrict__ runs, long long n_runs, long long* __restrict__ total_dev) {
    __shared__ long long wave_sums[TS_THREADS / 64];
    const long long all = scan_runs(runs, n_runs, wave_sums);
    if (threadIdx.x == 0) *total_dev = all;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_emit_kernel(const int2* __restrict__ vol, ExGeom g, long long n_vox,
                                                               const long long* __restrict__ run_offsets, float* __restrict__ points,
                                                               long long capacity) {
    __shared__ int wave_sums[TS_THREADS / 64];
    long long at = run_offsets[blockIdx.x];
    const long long base = (long long)blockIdx.x * EX_RUN;
    for (int r = 0; r < EX_RUN / TS_THREADS; ++r) {
        int ijk[3] = {0, 0, 0};
        int2 own = {0, 1}, nb[3] = {{0, 1}, {0, 1}, {0, 1}};
        const int m = tsdf_crossings(vol, g, base + r * TS_THREADS + threadIdx.x, n_vox, ijk, &own, nb);
        const int cnt = __popc(m);
        int total;
        const int incl = block_inclusive_scan(cnt, wave_sums, &total);
        if (m) {
            long long row = at + incl - cnt;
            const float c0 = tsdf_centre(g.lo[0], ijk[0], g.voxel), c1 = tsdf_centre(g.lo[1], ijk[1], g.voxel),
                        c2 = tsdf_centre(g.lo[2], ijk[2], g.voxel);
            const float D0 = (float)own.x / (float)own.y;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(m & (1 << a))) continue;
                const float D1 = (float)nb[a].x / (float)nb[a].y;
                const float t = D0 / (D0 - D1);
                const float step = t * g.voxel;
                if (row < capacity) {
                    points[3 * row] = a == 0 ? c0 + step : c0;
                    points[3 * row + 1] = a == 1 ? c1 + step : c1;
                    points[3 * row + 2] = a == 2 ? c2 + step : c2;
                }
                ++row;
            }
        }
        at += total;
    }
}

// ---- statistics
__global__ __launch_bounds__(TS_THREADS) void tsdf_stats_partial_kernel(const int2* __restrict__ vol, long long n_vox, int min_weight,
                                                                        unsigned long long* __restrict__ rows) {
    long long cnt[ST_COUNTS] = {0, 0};                               // observed, usable
    for (long long v = (long long)blockIdx.x * TS_THREADS + threadIdx.x; v < n_vox; v += (long long)ST_BLOCKS * TS_THREADS) {
        const int2 sw = vol[v];
        cnt[0] += sw.y > 0 ? 1 : 0;
        cnt[1] += tsdf_usable(sw, min_weight) ? 1 : 0;
    }
    stat_row_store<0, ST_COUNTS>(nullptr, cnt, rows + (size_t)blockIdx.x * ST_COUNTS);
}

__global__ __launch_bounds__(64) void tsdf_stats_final_kernel(const unsigned long long* __restrict__ rows, long long* __restrict__ counts2) {
    if (threadIdx.x < ST_COUNTS) counts2[threadIdx.x] = (long long)stat_rows_fold(rows, ST_BLOCKS, ST_COUNTS, 0, threadIdx.x);
}

// ---- host side
int check_frames_shape(int H, int W, float tan_half_fov, float z_clip) {
    NBP_RETURN_IF(H < 1 || W < 1 || !(tan_half_fov > 0.f) || !isfinite(tan_half_fov) || !(z_clip > 0.f) || !isfinite(z_clip), NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > TS_MAX_PIXELS, NBP_E_SHAPE);
    return 0;
}

int check_fusion(float trunc, float max_depth) {
    NBP_RETURN_IF(!(trunc > 0.f) || !isfinite(trunc) || !(max_depth > 0.f), NBP_E_ARG);      // (max_depth may be +inf; a NaN fails)
    return 0;
}

void fill_item(TsdfItem& it, int* vol, const float* lo, float voxel, int nx, int ny, int nz, float trunc, float max_depth) {
    it.vol = (int2*)vol;
    for (int a = 0; a < 3; ++a) it.lo[a] = lo[a];
    it.voxel = voxel;
    it.nx = nx; it.ny = ny; it.nz = nz;
    it.n_frames = 0;
    it.trunc = trunc;
    it.scale = (float)TS_QUANT / trunc;
    it.max_depth = max_depth;
    it.pad = 0;
}

void fill_frames(TsdfItem& it, const float* const* frames, const float* cams, int n) {
    it.n_frames = n;
    for (int f = 0; f < TS_FRAMES; ++f) it.frame[f] = frames[f < n ? f : 0];
    cams_from_host(cams, n, it.cam, TS_FRAMES);
}

unsigned voxel_blocks(int nx, int ny, int nz) { return (unsigned)nbp_cdiv((long long)nx * ny * nz, TS_THREADS); }

}  // namespace

extern "C" int nbp_tsdf_integrate_f32(int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, const float* depth_or_null,
                                      const float* const* frames_host_or_null, int n, const float* cams_host, int H, int W,
                                      float tan_half_fov, float z_clip, float trunc, float max_depth, void* stream) {
    NBP_ENTER();
    int rc = check_geometry(vol, lo_host, voxel, nx, ny, nz);
    if (rc) return rc;
    NBP_RETURN_IF(!cams_host || n < 1 || (!depth_or_null) == (!frames_host_or_null), NBP_E_ARG);
    rc = check_frames_shape(H, W, tan_half_fov, z_clip);
    if (rc) return rc;
    rc = check_fusion(trunc, max_depth);
    if (rc) return rc;
    NBP_RETURN_IF(n > 65535, NBP_E_SHAPE);
    const size_t HW = (size_t)H * W, vol_bytes = (size_t)nx * ny * nz * 8;
    for (int f = 0; f < n; ++f) {
        const float* fr = depth_or_null ? depth_or_null + (size_t)f * HW : frames_host_or_null[f];
        NBP_RETURN_IF(!fr, NBP_E_ARG);
        NBP_RETURN_IF(ranges_overlap(vol, vol_bytes, fr, HW * 4), NBP_E_ARG);
    }
    TsdfItem it;
    fill_item(it, vol, lo_host, voxel, nx, ny, nz, trunc, max_depth);
    for (int f0 = 0; f0 < n; f0 += TS_FRAMES) {                      // (any grouping of the frames gives the same bits)
        const int nf = n - f0 < TS_FRAMES ? n - f0 : TS_FRAMES;
        const float* fr[TS_FRAMES];
        for (int f = 0; f < nf; ++f) fr[f] = depth_or_null ? depth_or_null + (size_t)(f0 + f) * HW : frames_host_or_null[f0 + f];
        fill_frames(it, fr, cams_host + 12 * (size_t)f0, nf);
        tsdf_integrate_kernel<<<voxel_blocks(nx, ny, nz), TS_THREADS, 0, (hipStream_t)stream>>>(it, H, W, tan_half_fov, z_clip);
        rc = nbp_launch_status();
        if (rc) return rc;
    }
    return 0;
}

extern "C" int nbp_tsdf_integrate_batch_f32(int n_items, int* const* vols_host, const float* lo_host, const float* voxel_host,
                                            const int* dims_host, const float* trunc_host, const float* max_depth_host,
                                            const int* n_frames_host, const float* const* frames_host, const float* cams_host, int H,
                                            int W, float tan_half_fov, float z_clip, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(n_items < 1 || !vols_host || !lo_host || !voxel_host || !dims_host || !trunc_host || !max_depth_host || !n_frames_host ||
                      !frames_host || !cams_host,
                  NBP_E_ARG);
    NBP_RETURN_IF(n_items > TS_ITEMS, NBP_E_SHAPE);
    int rc = check_frames_shape(H, W, tan_half_fov, z_clip);
    if (rc) return rc;
    const size_t HW = (size_t)H * W;
    TsdfBatch b;
    unsigned blocks = 1;
    for (int i = 0; i < n_items; ++i) {
        const int* d = dims_host + 3 * i;
        rc = check_geometry(vols_host[i], lo_host + 3 * i, voxel_host[i], d[0], d[1], d[2]);
        if (rc) return rc;
        rc = check_fusion(trunc_host[i], max_depth_host[i]);
        if (rc) return rc;
        const int nf = n_frames_host[i];
        NBP_RETURN_IF(nf < 1, NBP_E_ARG);
        NBP_RETURN_IF(nf > TS_FRAMES, NBP_E_SHAPE);
        const size_t vol_bytes = (size_t)d[0] * d[1] * d[2] * 8;
        for (int g = 0; g < i; ++g) {                                // a voxel has ONE owner: no volume twice in a launch
            const int* e = dims_host + 3 * g;
            NBP_RETURN_IF(ranges_overlap(vols_host[i], vol_bytes, vols_host[g], (size_t)e[0] * e[1] * e[2] * 8), NBP_E_ARG);
        }
        for (int f = 0; f < nf; ++f) NBP_RETURN_IF(!frames_host[TS_FRAMES * i + f], NBP_E_ARG);
    }
    for (int i = 0; i < n_items; ++i) {                              // no frame of the launch inside a volume of the launch
        const int* d = dims_host + 3 * i;
        const size_t vol_bytes = (size_t)d[0] * d[1] * d[2] * 8;
        for (int g = 0; g < n_items; ++g)
            for (int f = 0; f < n_frames_host[g]; ++f)
                NBP_RETURN_IF(ranges_overlap(vols_host[i], vol_bytes, frames_host[TS_FRAMES * g + f], HW * 4), NBP_E_ARG);
    }
    for (int i = 0; i < TS_ITEMS; ++i) {
        const int q = i < n_items ? i : 0;
        const int* d = dims_host + 3 * q;
        fill_item(b.it[i], vols_host[q], lo_host + 3 * q, voxel_host[q], d[0], d[1], d[2], trunc_host[q], max_depth_host[q]);
        fill_frames(b.it[i], frames_host + TS_FRAMES * q, cams_host + 12 * TS_FRAMES * (size_t)q, n_frames_host[q]);
        if (i < n_items) {
            const unsigned nb = voxel_blocks(d[0], d[1], d[2]);
            blocks = nb > blocks ? nb : blocks;
        }
    }
    tsdf_integrate_batch_kernel<<<dim3(blocks, (unsigned)n_items), TS_THREADS, 0, (hipStream_t)stream>>>(b, H, W, tan_half_fov, z_clip);
    return nbp_launch_status();
}

extern "C" size_t nbp_tsdf_extract_workspace_bytes(long long n_voxels) {
    if (n_voxels < 1 || n_voxels > TS_MAX_VOXELS) return 0;
    return 256 + (size_t)extract_runs(n_voxels) * 8;
}

extern "C" int nbp_tsdf_extract_f32(const int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, int min_weight,
                                    float* points_or_null, long long capacity, long long* total, void* ws, size_t ws_bytes,
                                    void* stream) {
    NBP_ENTER();
    int rc = check_geometry(vol, lo_host, voxel, nx, ny, nz);
    if (rc) return rc;
    NBP_RETURN_IF(!total || !ws || min_weight < 1 || capacity < 0 || (capacity > 0 && !points_or_null), NBP_E_ARG);
    NBP_RETURN_IF(((uintptr_t)total & 7), NBP_E_SHAPE);
    const long long n_vox = (long long)nx * ny * nz;
    NBP_RETURN_IF(ws_bytes < nbp_tsdf_extract_workspace_bytes(n_vox), NBP_E_WS);
    const size_t vol_bytes = (size_t)n_vox * 8;
    long long* runs = (long long*)(((uintptr_t)ws + 255) / 256 * 256);
    const long long n_runs = extract_runs(n_vox);
    NBP_RETURN_IF(ranges_overlap(vol, vol_bytes, total, 8) || ranges_overlap(vol, vol_bytes, runs, (size_t)n_runs * 8) ||
                      ranges_overlap(runs, (size_t)n_runs * 8, total, 8),
                  NBP_E_ARG);
    if (capacity > 0)
        NBP_RETURN_IF(ranges_overlap(vol, vol_bytes, points_or_null, (size_t)capacity * 12) ||
                          ranges_overlap(points_or_null, (size_t)capacity * 12, total, 8) ||
                          ranges_overlap(points_or_null, (size_t)capacity * 12, runs, (size_t)n_runs * 8),
                      NBP_E_ARG);
    hipStream_t st = (hipStream_t)stream;
    ExGeom g = {{lo_host[0], lo_host[1], lo_host[2]}, voxel, nx, ny, nz, min_weight};
    tsdf_count_kernel<<<(unsigned)n_runs, TS_THREADS, 0, st>>>((const int2*)vol, g, n_vox, runs);
    rc = nbp_launch_status();
    if (rc) return rc;
    tsdf_scan_kernel<<<1, TS_THREADS, 0, st>>>(runs, n_runs, total);
    rc = nbp_launch_status();
    if (rc || capacity == 0) return rc;
    tsdf_emit_kernel<<<(unsigned)n_runs, TS_THREADS, 0, st>>>((const int2*)vol, g, n_vox, runs, points_or_null, capacity);
    return nbp_launch_status();
}

extern "C" size_t nbp_tsdf_stats_workspace_bytes(void) { return stat_rows_bytes(ST_BLOCKS, ST_COUNTS); }

extern "C" int nbp_tsdf_stats_i64(const int* vol, long long n_voxels, int min_weight, long long* counts2, void* ws, size_t ws_bytes,
                                  void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!vol || !counts2 || !ws || n_voxels < 1 || min_weight < 1, NBP_E_ARG);
    NBP_RETURN_IF(n_voxels > TS_MAX_VOXELS || (((uintptr_t)vol | (uintptr_t)counts2) & 7), NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < nbp_tsdf_stats_workspace_bytes(), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* rows = carve(ws, stat_rows_layout, (size_t)ST_BLOCKS, ST_COUNTS);
    tsdf_stats_partial_kernel<<<ST_BLOCKS, TS_THREADS, 0, st>>>((const int2*)vol, n_voxels, min_weight, rows);
    const int rc = nbp_launch_status();
    if (rc) return rc;
    tsdf_stats_final_kernel<<<1, 64, 0, st>>>(rows, counts2);
    return nbp_launch_status();
}
