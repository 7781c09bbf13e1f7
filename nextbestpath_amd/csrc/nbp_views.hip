// nbp_views.hip -- held-out view metrics: a point-splat render of a coloured cloud that is already on the device, and its
// pixel-by-pixel comparison with the mesh render of the same poses (include/nbp_hip.h: nbp_views_*; the definition of record is
// nextbestpath_amd/utility/view_metrics.py).  Not in the reference.
//
// Splat.  One thread per point reads the point once and loops over the <= 8 cameras of a launch (they travel in the kernel
// arguments, as nbp_camera.h's CamSet; more views go in chunks of 8).  The projection is nbp_camera.h's `project`, the inverse of
// unproject_pixel's NDC tables: bit for bit view_metrics.project.  A point covers the
// (2 r + 1)^2 pixels around its own, clipped to the image; each pixel keeps the smallest key (float bits of v2) << 32 | index by
// a 64-bit atomicMin (v2 > z_clip > 0: positive floats order like their bits), the rasteriser's merge.  A minimum is blind to
// arrival order: two runs give the same bits, and a cloud splatted in parts (each at its own rows: the index is the row) gives
// the bits of the whole.  Before the atomic the pixel is read plainly and the atomic skipped where the stored key is already <=
// the thread's: the buffer only ever decreases, so a stale read (another XCD's L2) costs a redundant atomic, never a missed one.
//
// Statistics.  One pass over the pixels resolves the keys, classifies and reduces by nbp_stat_rows.h's fixed-order fold (VS_BLOCKS
// blocks per view, a row being three float64 sums and six counts).  No floating-point atomics: two runs give the same bits.
#include "common.h"
#include "nbp_camera.h"
#include "nbp_stat_rows.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int VIEW_CAMS = MAX_CAMS;              // cameras of one splat launch
constexpr int VIEW_MAX_RADIUS = 4;
constexpr long long VIEW_MAX_PIXELS = 1ll << 29;
constexpr long long VIEW_MAX_POINTS = 0xffffffffll;   // fewer than this: the key's low word is the point's index
constexpr int VIEW_MAX_VIEWS = 65535;            // the statistics' grid.y
constexpr int VS_BLOCKS = 32, VS_THREADS = STAT_THREADS;
constexpr int VS_SUMS = 3, VS_COUNTS = 6, VS_ROW = VS_SUMS + VS_COUNTS;      // 8-byte words of a row: the sums, then the counts
constexpr unsigned long long VIEW_EMPTY = ~0ull;

template <bool PRECHECK>
__global__ __launch_bounds__(256) void views_splat_kernel(const float* __restrict__ cloud, const long long* __restrict__ n_dev,
                                                          long long n_host, CamSet cams, int n_cams, int H, int W, int radius,
                                                          float tanh_fov, float z_clip, float z_far,
                                                          unsigned long long* __restrict__ keys) {
    long long n = n_dev ? *n_dev : n_host;
    n = n < 0 ? 0 : (n > n_host ? n_host : n);                       // rows at or beyond the device count are never read
    const NdcTables nt(H, W);
    const float r_lo = (float)-radius, row_hi = (float)(H - 1 + radius), col_hi = (float)(W - 1 + radius);
    const size_t HW = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float p[3] = {cloud[3 * i], cloud[3 * i + 1], cloud[3 * i + 2]};
        for (int c = 0; c < n_cams; ++c) {
            float fr, fc, v2;
            if (!project(p, cams.c[c], nt, tanh_fov, z_clip, z_far, &fr, &fc, &v2)) continue;
            // the footprint misses the image (decided on the FLOATS: only an in-range value reaches the int conversion)
            if (!(fr >= r_lo && fr <= row_hi && fc >= r_lo && fc <= col_hi)) continue;
            const int row = (int)fr, col = (int)fc;
            const int r0 = max(row - radius, 0), r1 = min(row + radius, H - 1);
            const int c0 = max(col - radius, 0), c1 = min(col + radius, W - 1);
            const unsigned long long key = ((unsigned long long)__float_as_uint(v2) << 32) | (unsigned long long)(unsigned)i;
            unsigned long long* img = keys + (size_t)c * HW;
            for (int rr = r0; rr <= r1; ++rr)
                for (int cc = c0; cc <= c1; ++cc) {
                    unsigned long long* px = img + (size_t)rr * W + cc;
                    if (PRECHECK) {
                        if (*px > key) atomicMin(px, key);
                    } else {
                        atomicMin(px, key);
                    }
                }
        }
    }
}

// ---- resolve
__global__ __launch_bounds__(256) void views_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ cloud_rgb,
                                                            long long n_cloud, size_t n_pix, float* __restrict__ z_c,
                                                            float* __restrict__ rgb_c, long long* __restrict__ index) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long k = keys[i];
        const long long idx = (long long)(k & 0xffffffffull);
        const bool filled = k != VIEW_EMPTY && idx < n_cloud;       // (an index beyond the cloud's rows reads as empty: never dereferenced)
        if (z_c) z_c[i] = filled ? __uint_as_float((unsigned)(k >> 32)) : -1.f;
        if (index) index[i] = filled ? idx : -1;
        if (rgb_c) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb_c[3 * i + ch] = filled ? cloud_rgb[3 * (size_t)idx + ch] : 0.f;
        }
    }
}

// ---- resolve + classify + reduce: grid (VS_BLOCKS, n_views)
__global__ __launch_bounds__(VS_THREADS) void views_partial_kernel(const unsigned long long* __restrict__ keys,
                                                                  const float* __restrict__ cloud_rgb, long long n_cloud,
                                                                  const float* __restrict__ z_gt, const float* __restrict__ rgb_gt,
                                                                  int HW, float tau, float z_far, unsigned long long* __restrict__ rows) {
    const int view = blockIdx.y;
    const size_t base = (size_t)view * HW;
    long long cnt[VS_COUNTS];
    double sum[VS_SUMS];
#pragma unroll
    for (int k = 0; k < VS_COUNTS; ++k) cnt[k] = 0;
#pragma unroll
    for (int k = 0; k < VS_SUMS; ++k) sum[k] = 0.0;
    const bool colours = cloud_rgb && rgb_gt;
    for (int p = blockIdx.x * VS_THREADS + threadIdx.x; p < HW; p += VS_BLOCKS * VS_THREADS) {
        const unsigned long long k = keys[base + p];
        const long long idx = (long long)(k & 0xffffffffull);
        const bool c = k != VIEW_EMPTY && idx < n_cloud;
        const float zg = z_gt[base + p];
        const bool gt = zg > -1.f && zg < z_far;
        const float zc = c ? __uint_as_float((unsigned)(k >> 32)) : -1.f;
        const float dz = zc - zg;
        const bool hit = gt && c && fabsf(dz) <= tau;
        cnt[0] += gt ? 1 : 0;
        cnt[1] += c ? 1 : 0;
        cnt[2] += hit ? 1 : 0;
        cnt[3] += gt && !c ? 1 : 0;
        cnt[4] += gt && c && dz > tau ? 1 : 0;
        cnt[5] += c && (!gt || dz < -tau) ? 1 : 0;
        if (hit) {
            const double d = (double)zc - (double)zg;
            sum[0] += fabs(d);
            sum[1] += d * d;
            if (colours) {
                const float* a = cloud_rgb + 3 * (size_t)idx;
                const float* b = rgb_gt + 3 * (base + p);
                const double d0 = (double)a[0] - (double)b[0], d1 = (double)a[1] - (double)b[1], d2 = (double)a[2] - (double)b[2];
                sum[2] += (d0 * d0 + d1 * d1) + d2 * d2;
            }
        }
    }
    stat_row_store<VS_SUMS, VS_COUNTS>(sum, cnt, rows + ((size_t)view * VS_BLOCKS + blockIdx.x) * VS_ROW);
}

// one block per view: the view's rows added in index order
__global__ __launch_bounds__(64) void views_final_kernel(const unsigned long long* __restrict__ rows, long long* __restrict__ counts,
                                                         double* __restrict__ sums) {
    const int view = blockIdx.x, col = threadIdx.x;
    const unsigned long long* r = rows + (size_t)view * VS_BLOCKS * VS_ROW;
    if (col >= VS_ROW) return;
    const unsigned long long total = stat_rows_fold(r, VS_BLOCKS, VS_ROW, VS_SUMS, col);
    if (col < VS_SUMS) sums[(size_t)view * VS_SUMS + col] = __longlong_as_double((long long)total);
    else counts[(size_t)view * VS_COUNTS + (col - VS_SUMS)] = (long long)total;
}

bool views_shape_ok(int n_views, int H, int W) {
    return n_views >= 1 && H >= 2 && W >= 2;                         // (min(H, W) - 1 divides nothing, but scales everything to 0)
}

}  // namespace

extern "C" int nbp_views_splat_f32(const float* cloud3, long long n, const long long* n_dev_or_null, const float* cams_host, int n_views,
                                   int H, int W, int radius, float tan_half_fov, float z_clip, float z_far, int accumulate,
                                   int precheck, unsigned long long* keys, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!keys || !cams_host || n < 0 || (n > 0 && !cloud3) || !views_shape_ok(n_views, H, W), NBP_E_ARG);
    NBP_RETURN_IF(radius < 0 || radius > VIEW_MAX_RADIUS || !(tan_half_fov > 0) || !(z_clip > 0) || !(z_far > z_clip), NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > VIEW_MAX_PIXELS || n >= VIEW_MAX_POINTS, NBP_E_SHAPE);
    NBP_RETURN_IF(((uintptr_t)keys & 7), NBP_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)n_views * HW * 8, st);
        if (e != hipSuccess) return (int)e;
    }
    if (n == 0) return 0;
    const int grid = nbp_ew_grid(n, 256);
    for (int v0 = 0; v0 < n_views; v0 += VIEW_CAMS) {
        const int nc = n_views - v0 < VIEW_CAMS ? n_views - v0 : VIEW_CAMS;
        CamSet cs;
        cams_from_host(cams_host + 12 * (size_t)v0, nc, cs.c, VIEW_CAMS);
        unsigned long long* dst = keys + (size_t)v0 * HW;
        if (precheck)
            views_splat_kernel<true><<<grid, 256, 0, st>>>(cloud3, n_dev_or_null, n, cs, nc, H, W, radius, tan_half_fov, z_clip, z_far, dst);
        else
            views_splat_kernel<false><<<grid, 256, 0, st>>>(cloud3, n_dev_or_null, n, cs, nc, H, W, radius, tan_half_fov, z_clip, z_far, dst);
        const int rc = nbp_launch_status();
        if (rc) return rc;
    }
    return 0;
}

extern "C" int nbp_views_resolve_f32(const unsigned long long* keys, const float* cloud_rgb_or_null, long long n_cloud, int n_views, int H,
                                     int W, float* z_c_or_null, float* rgb_c_or_null, long long* index_or_null, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!keys || n_cloud < 0 || !views_shape_ok(n_views, H, W) || (rgb_c_or_null && !cloud_rgb_or_null), NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > VIEW_MAX_PIXELS || n_cloud >= VIEW_MAX_POINTS, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)keys | (uintptr_t)index_or_null) & 7), NBP_E_SHAPE);
    const size_t n_pix = (size_t)n_views * H * W;
    views_resolve_kernel<<<nbp_ew_grid((long long)n_pix, 256), 256, 0, (hipStream_t)stream>>>(keys, cloud_rgb_or_null, n_cloud, n_pix,
                                                                                             z_c_or_null, rgb_c_or_null, index_or_null);
    return nbp_launch_status();
}

extern "C" size_t nbp_views_stats_workspace_bytes(int n_views) {
    if (n_views < 1 || n_views > VIEW_MAX_VIEWS) return 0;
    return stat_rows_bytes((size_t)n_views * VS_BLOCKS, VS_ROW);
}

extern "C" int nbp_views_stats_f64(const unsigned long long* keys, const float* cloud_rgb_or_null, long long n_cloud, const float* z_gt,
                                   const float* rgb_gt_or_null, int n_views, int H, int W, float depth_tolerance, float z_far,
                                   long long* counts6, double* sums3, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!keys || !z_gt || !counts6 || !sums3 || !ws || n_cloud < 0 || !views_shape_ok(n_views, H, W), NBP_E_ARG);
    NBP_RETURN_IF(!(depth_tolerance >= 0) || !isfinite(depth_tolerance) || !(z_far > 0), NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > VIEW_MAX_PIXELS || n_cloud >= VIEW_MAX_POINTS || n_views > VIEW_MAX_VIEWS, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)keys | (uintptr_t)counts6 | (uintptr_t)sums3) & 7), NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < nbp_views_stats_workspace_bytes(n_views), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* rows = carve(ws, stat_rows_layout, (size_t)n_views * VS_BLOCKS, VS_ROW);
    views_partial_kernel<<<dim3(VS_BLOCKS, (unsigned)n_views), VS_THREADS, 0, st>>>(keys, cloud_rgb_or_null, n_cloud, z_gt, rgb_gt_or_null,
                                                                                   H * W, depth_tolerance, z_far, rows);
    const int rc = nbp_launch_status();
    if (rc) return rc;
    views_final_kernel<<<(unsigned)n_views, 64, 0, st>>>(rows, counts6, sums3);
    return nbp_launch_status();
}
