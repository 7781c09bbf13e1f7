// nbp_camera.h -- the pinhole camera of the device code, once: a camera (R, T) and its view transform, the two pixel <-> NDC
// conventions by name, the projection of a point to a pixel, and the host packing of cameras into kernel arguments.  Every
// expression here is fp32 with one rounding per operation, in an order that is a contract with a numpy definition (oracle/camera.py,
// oracle/raster.py, utility/view_metrics.py::project).  Included inside each translation unit (anonymous namespace),
// like nbp_carve.h; not part of the C ABI.
#pragma once
#include <math.h>
#include <stddef.h>

// no contraction from here to the end of the including file (device code would otherwise fuse a multiply into the add behind it)
#pragma clang fp contract(off)

namespace {

struct Cam { float R[9]; float T[3]; };   // R row-major; X_view = X_world R + T (row vector)
constexpr int MAX_CAMS = 8;
struct CamSet { Cam c[MAX_CAMS]; };       // cameras travel in the kernel arguments (no H2D copy, no sync)

__device__ __forceinline__ void to_view(const float* p, const float* R, const float* T, float* o) {
    // X_view = X_world R + T (row vector): o_j = sum_k p_k R[k][j] + T_j
    o[0] = ((p[0] * R[0] + p[1] * R[3]) + p[2] * R[6]) + T[0];
    o[1] = ((p[0] * R[1] + p[1] * R[4]) + p[2] * R[7]) + T[1];
    o[2] = ((p[0] * R[2] + p[1] * R[5]) + p[2] * R[8]) + T[2];
}

// camera centre C = -T R^T
__device__ __forceinline__ void cam_centre(const Cam& cam, float* c) {
    c[0] = -((cam.T[0] * cam.R[0] + cam.T[1] * cam.R[1]) + cam.T[2] * cam.R[2]);
    c[1] = -((cam.T[0] * cam.R[3] + cam.T[1] * cam.R[4]) + cam.T[2] * cam.R[5]);
    c[2] = -((cam.T[0] * cam.R[6] + cam.T[1] * cam.R[7]) + cam.T[2] * cam.R[8]);
}

// ---- convention 1, the reference's NDC TABLES (macarons_utils.py:2270-2279): with s = min(H, W), column col has
// ndc_x = f32(W / s) - col / (s - 1) * 2 and row `row` has ndc_y = f32(H / s) - row / (s - 1) * 2 (+X left, +Y up).  The
// un-projection, the field-of-view bounds and the projection of a point to a pixel use it: an un-projected pixel projects onto itself.
// n = W and i = a column for ndc_x, n = H and i = a row for ndc_y; ndc_table_max is the table's entry 0, its largest
__device__ __forceinline__ float ndc_table_max(int n, int s) { return (float)((double)n / s); }
__device__ __forceinline__ float ndc_table_at(int n, int s, int i) { return ndc_table_max(n, s) - ((float)i / (float)(s - 1)) * 2.f; }

// Pixel (row, col) with view-space depth z -> world point (oracle/camera.py)
__device__ __forceinline__ void unproject_pixel(int row, int col, float z, int H, int W, float tanh_fov,
                                                const float* R, const float* T, float* out) {
    const int s = H < W ? H : W;
    const float ndc_x = ndc_table_at(W, s, col);                     // ref mu:2272-2274
    const float ndc_y = ndc_table_at(H, s, row);                     // ref mu:2275-2277
    const float xv = (ndc_x * z) * tanh_fov;
    const float yv = (ndc_y * z) * tanh_fov;
    const float dx = xv - T[0], dy = yv - T[1], dz = z - T[2];
    // X_world = (X_view - T) R^T  (row vectors)
    out[0] = (dx * R[0] + dy * R[1]) + dz * R[2];
    out[1] = (dx * R[3] + dy * R[4]) + dz * R[5];
    out[2] = (dx * R[6] + dy * R[7]) + dz * R[8];
}

// what the projection needs of the tables, made once per thread: entry 0 of either table and f32(s - 1)
struct NdcTables {
    float max_x, max_y, sm1;
    __device__ __forceinline__ NdcTables(int H, int W) {
        const int s = H < W ? H : W;
        max_x = ndc_table_max(W, s);
        max_y = ndc_table_max(H, s);
        sm1 = (float)(s - 1);
    }
};

// view_metrics.project, step by step: point -> view-space point -> takes part iff z_clip < v2 < z_far and the NDC are finite
// -> float row and column floor(. + 0.5) (not yet integers: they may be far outside the image; the caller's range test decides on
// the FLOATS, so that only an in-range value reaches an int conversion) and v2.  nt = NdcTables(H, W), made once by the caller.
__device__ __forceinline__ bool project(const float* p, const Cam& cam, const NdcTables& nt, float tanh_fov, float z_clip, float z_far,
                                        float* row, float* col, float* v2) {
    float v[3];
    to_view(p, cam.R, cam.T, v);
    *v2 = v[2];
    if (!(v[2] > z_clip && v[2] < z_far)) return false;              // (a NaN fails both)
    const float t = v[2] * tanh_fov;
    const float nx = v[0] / t, ny = v[1] / t;
    if (!(isfinite(nx) && isfinite(ny))) return false;
    *col = floorf(((nt.max_x - nx) * 0.5f) * nt.sm1 + 0.5f);
    *row = floorf(((nt.max_y - ny) * 0.5f) * nt.sm1 + 0.5f);
    return true;
}

// ---- convention 2, the rasteriser's PIXEL CENTRES (oracle/raster.py): pixel (row, col) is seen along the view-space ray
// (dx, dy, 1) = (ndc_x tan_half_fov, ndc_y tan_half_fov, 1) with ndc_x = (W - (2 col + 1)) / s and ndc_y = (H - (2 row + 1)) / s:
// pixel_centre_ndc with n = W, i = col and with n = H, i = row.  The tile kernel and the shading cast this ray; raster_setup's
// `emit` inverts it (col = (W - s nx - 1) / 2) for a face's screen box.
__device__ __forceinline__ float pixel_centre_ndc(int n, int s, int i) { return ((float)n - (2.f * i + 1.f)) / (float)s; }

// ---- host: n <= n_slots cameras [n][12] (R row-major (9) then T (3)) into slots[0..n_slots); the slots at or beyond n are zero
// (no kernel reads them: each indexes or loops below its own camera count) and nothing beyond cams12[12 n) is read
void cams_from_host(const float* cams12, int n, Cam* slots, int n_slots) {
    for (int f = 0; f < n_slots; ++f)
        for (int k = 0; k < 12; ++k) {
            const float v = f < n ? cams12[12 * (size_t)f + k] : 0.f;
            if (k < 9) slots[f].R[k] = v; else slots[f].T[k - 9] = v;
        }
}

}  // namespace
