// nbp_depth_filter.hip -- the depth-frame filter: gated median, speckle rejection, hole filling (include/nbp_hip.h:
// nbp_depth_filter_f32, nbp_depth_filter_batch_f32; the definition, which this file equals bit for bit, is
// nextbestpath_amd/utility/depth_filter.py).
//
// Raw frame -> filtered frame, out of place (every decision reads raw neighbours).  A workgroup owns a 32 x 32 tile of one frame
// (blockIdx.z = frame, blockIdx.x = the tile, row-major) and keeps it with a halo of `radius` pixels in LDS; cells outside the image
// are stored as -1, which is "invalid".  One lane owns 4 consecutive pixels of a tile row: 16-byte loads and stores when the frames
// lie on the 16-byte grid and W % 4 == 0 (then a quad is inside the image or outside it as a whole), 4-byte accesses for any other
// H, W >= 1; the halo is 4-byte loads.  A tile row is 32 + 2 radius + 1 floats: with the odd pitch the 8 lanes x 4 rows of a
// 32-lane group read 32 different banks.
// Selection is by counting over the window, in fully unrolled loops with compile-time indices (the window lives in registers, never
// in a runtime-indexed array): pixels that take no part hold NaN, for which `<=` is false, so they are never counted and never
// chosen; the answer is the smallest candidate with at least rank + 1 members <= it.  (2 radius + 1)^4 compares per pixel: 81 or 625.
// One launch, no workspace, no atomics.  8 H W bytes of traffic per frame.
#include "common.h"

#pragma clang fp contract(off)      // the gate's three fp32 operations, each rounded on its own

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_TW = 32, DF_TH = 32;              // the tile: 8 lanes of 4 pixels x 32 rows
constexpr int DF_ITEMS = 12;                       // the step's group stages chunk at 12 items (nbp_sim.hip: STEP_BATCH) ...
constexpr int DF_FRAMES = 4 * DF_ITEMS;            // ... of <= 4 frames each

struct FilterSpec { float range_base, range_quad; int smooth, min_support, fill_support; };
struct FilterBatch { const float* raw[DF_FRAMES]; float* out[DF_FRAMES]; };

__device__ __forceinline__ float gate(float c, const FilterSpec& sp) {
    float t = c * c;
    t = sp.range_quad * t;
    t = sp.range_base + t;
    return t;
}

// the filtered value of the pixel whose window's top-left cell is win[0] (tile rows are PITCH floats apart)
template <int R, int PITCH>
__device__ __forceinline__ float filter_pixel(const float* win, const FilterSpec& sp) {
    constexpr int D = 2 * R + 1, K = D * D, C = R * D + R;
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = win[(k / D) * PITCH + (k % D)];
    const float z = w[C];
    const bool centre = z > -1.0f;
    if (!centre && sp.fill_support == 0) return -1.0f;
    const float tau = gate(z, sp);
    const float nan = __builtin_nanf("");
    int n = 0;                                     // |S| of a valid centre, |V| of an invalid one
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k == C) continue;
        const float v = w[k];
        const bool member = v > -1.0f && (!centre || fabsf(v - z) <= tau);
        n += member ? 1 : 0;
        w[k] = member ? v : nan;
    }
    int need;                                      // rank + 1
    if (centre) {
        if (n < sp.min_support) return -1.0f;
        if (!sp.smooth) return z;
        need = n / 2 + 1;
    } else {
        if (n < sp.fill_support) return -1.0f;     // (fill_support >= 1 here: n >= 1)
        w[C] = nan;
        need = (n - 1) / 2 + 1;
    }
    float best = __builtin_inff();
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float c = w[i];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) cnt += w[k] <= c ? 1 : 0;
        if (cnt >= need && c < best) best = c;
    }
    if (centre) return best;
    const float tau_m = gate(best, sp);            // no fill across a depth edge: every valid neighbour within the gate of m = best
    bool edge = false;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (k != C) edge = edge || (w[k] > -1.0f && !(fabsf(w[k] - best) <= tau_m));
    return edge ? -1.0f : best;
}

// ONE body for both launch forms: tile blockIdx.x of one [H][W] frame
template <int R>
__device__ __forceinline__ void filter_tile(const float* __restrict__ raw, float* __restrict__ out, int H, int W, unsigned tiles_x,
                                            const FilterSpec& sp, bool vec, float* tile) {
    constexpr int HALO_W = DF_TW + 2 * R, PITCH = HALO_W + 1;
    constexpr int TOP_BOTTOM = 2 * R * HALO_W, N_HALO = TOP_BOTTOM + DF_TH * 2 * R;
    const int tid = threadIdx.x, tx = tid & 7, ty = tid >> 3;
    const unsigned by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = (int)bx * DF_TW, y0 = (int)by * DF_TH;
    const int gx = x0 + 4 * tx, gy = y0 + ty;      // this lane's quad
    const size_t p0 = (size_t)gy * W + gx;
    {
        f32x4 c = {-1.0f, -1.0f, -1.0f, -1.0f};
        if (gy < H) {
            if (vec) {
                if (gx < W) c = *(const f32x4*)(raw + p0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx + j < W) c[j] = raw[p0 + j];
            }
        }
        float* own = tile + (ty + R) * PITCH + R + 4 * tx;
#pragma unroll
        for (int j = 0; j < 4; ++j) own[j] = c[j];
    }
    for (int i = tid; i < N_HALO; i += DF_THREADS) {       // R rows above, R below, then R columns either side of the 32 rows
        int lr, lc;
        if (i < TOP_BOTTOM) {
            lr = i / HALO_W;
            lc = i - lr * HALO_W;
            if (lr >= R) lr += DF_TH;
        } else {
            const int s = i - TOP_BOTTOM;
            lr = R + s / (2 * R);
            lc = s % (2 * R);
            if (lc >= R) lc += DF_TW;
        }
        const int yy = y0 + lr - R, xx = x0 + lc - R;
        float v = -1.0f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = raw[(size_t)yy * W + xx];
        tile[lr * PITCH + lc] = v;
    }
    __syncthreads();
    if (gy >= H || gx >= W) return;
    const float* win = tile + ty * PITCH + 4 * tx;         // the window of the quad's first pixel starts R up and R left of it
    float o0 = -1.0f, o1 = -1.0f, o2 = -1.0f, o3 = -1.0f;
    constexpr int COPIES = R == 1 ? 4 : 1;                 // (the 5 x 5 selection is 625 compares: one copy of it, not four)
#pragma unroll COPIES
    for (int j = 0; j < 4; ++j) {
        const float f = filter_pixel<R, PITCH>(win + j, sp);
        o0 = j == 0 ? f : o0;
        o1 = j == 1 ? f : o1;
        o2 = j == 2 ? f : o2;
        o3 = j == 3 ? f : o3;
    }
    if (vec) {
        const f32x4 o = {o0, o1, o2, o3};
        *(f32x4*)(out + p0) = o;
        return;
    }
    out[p0] = o0;
    if (gx + 1 < W) out[p0 + 1] = o1;
    if (gx + 2 < W) out[p0 + 2] = o2;
    if (gx + 3 < W) out[p0 + 3] = o3;
}

template <int R>
constexpr int tile_floats() { return (DF_TH + 2 * R) * (DF_TW + 2 * R + 1); }

// n consecutive frames: frame blockIdx.z
template <int R>
__global__ __launch_bounds__(DF_THREADS) void depth_filter_kernel(const float* __restrict__ raw, float* __restrict__ out, int H, int W,
                                                                  unsigned HW, unsigned tiles_x, FilterSpec sp, int vec) {
    __shared__ __attribute__((aligned(16))) float tile[tile_floats<R>()];
    const size_t off = (size_t)blockIdx.z * HW;
    filter_tile<R>(raw + off, out + off, H, W, tiles_x, sp, vec != 0, tile);
}

// frame blockIdx.z of the batch: its own pointers, which are kernel arguments
template <int R>
__global__ __launch_bounds__(DF_THREADS) void depth_filter_batch_kernel(FilterBatch b, int H, int W, unsigned tiles_x, FilterSpec sp,
                                                                        int vec) {
    __shared__ __attribute__((aligned(16))) float tile[tile_floats<R>()];
    const unsigned f = blockIdx.z;
    filter_tile<R>(b.raw[f], b.out[f], H, W, tiles_x, sp, vec != 0, tile);
}

// NBP_E_* of the arguments the two forms share, 0 when they are fine
int check_spec(int H, int W, int radius, float range_base, float range_quad, int min_support, int fill_support) {
    NBP_RETURN_IF(H < 1 || W < 1, NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > (1ll << 29), NBP_E_SHAPE);
    NBP_RETURN_IF(radius != 1 && radius != 2, NBP_E_ARG);
    NBP_RETURN_IF(!(range_base >= 0.f) || !(range_quad >= 0.f) || !(range_base > 0.f || range_quad > 0.f), NBP_E_ARG);
    const int top = (2 * radius + 1) * (2 * radius + 1) - 1;
    NBP_RETURN_IF(min_support < 0 || min_support > top || fill_support < 0 || fill_support > top, NBP_E_ARG);
    return 0;
}

bool overlap(const float* a, const float* b, size_t n) { return a < b + n && b < a + n; }

unsigned tiles_along(int n, int tile) { return (unsigned)nbp_cdiv(n, tile); }

}  // namespace

extern "C" int nbp_depth_filter_f32(const float* raw, float* out, int n, int H, int W, int radius, float range_base, float range_quad,
                                    int smooth, int min_support, int fill_support, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!raw || !out || n < 1, NBP_E_ARG);
    int rc = check_spec(H, W, radius, range_base, range_quad, min_support, fill_support);
    if (rc) return rc;
    NBP_RETURN_IF(n > 65535, NBP_E_SHAPE);
    const unsigned HW = (unsigned)H * (unsigned)W;
    NBP_RETURN_IF(overlap(raw, out, (size_t)n * HW), NBP_E_ARG);                 // out of place: every decision reads raw neighbours
    const FilterSpec sp = {range_base, range_quad, smooth != 0, min_support, fill_support};
    const int vec = W % 4 == 0 && (((uintptr_t)raw | (uintptr_t)out) & 15) == 0;
    const unsigned tiles_x = tiles_along(W, DF_TW);
    dim3 grid(tiles_x * tiles_along(H, DF_TH), 1, (unsigned)n);
    if (radius == 1)
        depth_filter_kernel<1><<<grid, DF_THREADS, 0, (hipStream_t)stream>>>(raw, out, H, W, HW, tiles_x, sp, vec);
    else
        depth_filter_kernel<2><<<grid, DF_THREADS, 0, (hipStream_t)stream>>>(raw, out, H, W, HW, tiles_x, sp, vec);
    return nbp_launch_status();
}

extern "C" int nbp_depth_filter_batch_f32(int n, const float* const* raw, float* const* out, int H, int W, int radius, float range_base,
                                          float range_quad, int smooth, int min_support, int fill_support, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(n < 1 || !raw || !out, NBP_E_ARG);
    NBP_RETURN_IF(n > DF_FRAMES, NBP_E_SHAPE);
    int rc = check_spec(H, W, radius, range_base, range_quad, min_support, fill_support);
    if (rc) return rc;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const FilterSpec sp = {range_base, range_quad, smooth != 0, min_support, fill_support};
    FilterBatch b;
    int vec = W % 4 == 0;
    for (int f = 0; f < n; ++f) {
        NBP_RETURN_IF(!raw[f] || !out[f], NBP_E_ARG);
        for (int g = 0; g < n; ++g) NBP_RETURN_IF(raw[g] && overlap(raw[g], out[f], HW), NBP_E_ARG);
        for (int g = 0; g < f; ++g) NBP_RETURN_IF(overlap(out[g], out[f], HW), NBP_E_ARG);
        if ((((uintptr_t)raw[f] | (uintptr_t)out[f]) & 15) != 0) vec = 0;
    }
    for (int f = 0; f < DF_FRAMES; ++f) {
        const int q = f < n ? f : 0;
        b.raw[f] = raw[q]; b.out[f] = out[q];
    }
    const unsigned tiles_x = tiles_along(W, DF_TW);
    dim3 grid(tiles_x * tiles_along(H, DF_TH), 1, (unsigned)n);
    if (radius == 1)
        depth_filter_batch_kernel<1><<<grid, DF_THREADS, 0, (hipStream_t)stream>>>(b, H, W, tiles_x, sp, vec);
    else
        depth_filter_batch_kernel<2><<<grid, DF_THREADS, 0, (hipStream_t)stream>>>(b, H, W, tiles_x, sp, vec);
    return nbp_launch_status();
}
