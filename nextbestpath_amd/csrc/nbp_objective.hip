// nbp_objective.hip -- the training objective of one batch as ONE forward and ONE backward call, with the terms of every sample
// kept apart (include/nbp_hip.h: nbp_objective_*; the definition of record is nextbestpath_amd/utility/priority.py).
//
//   v_b = sum over the value targets of sample b of (out1[b,c,x,y] - gain)^2       n_b = the number of those targets
//   o_b = sum over the pixels of plane b of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))
//
// Every term is formed in fp32 exactly as loss_partial_kernel (nbp_train.hip) forms it and accumulated in double.
//
// Forward, launch 1 (partial_kernel, grid (G + 1, B)): workgroups 0 .. G-1 of a column stream plane b of out2 and gt, 16 bytes per
// lane where a plane is a whole number of aligned quads (4-byte accesses for what is left, or for all of it); G depends on S alone.
// A thread adds its own terms in index order, the workgroup adds its threads by a fixed tree (shuffles inside a wave, the four
// waves in order) and writes ONE partial into the workspace.  Workgroup G of the column owns the value targets of sample b: it
// scans the K rows in chunks of one row per thread, ranks the sample's rows IN ROW ORDER (ballot + popcount, the waves' counts
// through LDS) and adds the term of rank r into LDS slot r mod 256 -- the ranks of one chunk are distinct and fewer than 257, so no
// two threads meet in a slot -- then adds the slots by the same tree.  The order of every sum therefore depends on the sample's own
// data and on S only: not on B, not on the slot b, not on where the sample's rows sit among the others'.
// Forward, launch 2 (finish_kernel, one workgroup): o_b = the G partials in order; totals = sum_b w_b v_b, sum_b w_b o_b, a thread
// per sample (strided), the same tree.  No floating-point atomics anywhere in the forward: two runs give the same bits.
//
// Backward: one asynchronous fill (d_out1 = 0) and ONE launch (backward_kernel): the first B * G workgroups write
// d_out2 = coef1 w_b (p - t) / max(p (1 - p), 1e-12) / (B S^2) (the expression of loss_grad_kernel), the others scatter-add
// coef0 w_b 2 (pred - gain) / K into d_out1 with atomicAdd as scatter_values_kernel does (a cell named twice receives both).  The two
// coefficients are read from device memory: nothing waits for the host.
#include "common.h"

#include <stddef.h>

namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_WAVES = OBJ_THREADS / 64;
constexpr int OBJ_MAX_WGS = 16;                  // workgroups per sample plane, at most

// workgroups per plane: one per 1024 pixels (a 16-byte access per thread), a function of S alone
inline int obj_wgs(int S) {
    long long g = nbp_cdiv((long long)S * S, 4 * OBJ_THREADS);
    if (g < 1) g = 1;
    if (g > OBJ_MAX_WGS) g = OBJ_MAX_WGS;
    return (int)g;
}

// quads per plane that may be read 16 bytes at a time: all of them when every plane starts on a 16-byte boundary, else none
inline int obj_quads(int S, const void* a, const void* b, const void* c) {
    const long long n = (long long)S * S;
    uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
    if (c) bits |= (uintptr_t)c;
    return (n % 4 == 0 && (bits & 15) == 0) ? (int)(n / 4) : 0;
}

// the sum over the workgroup's threads, to every thread: shuffles inside a wave, then the waves in order
__device__ __forceinline__ double block_sum(double s, double* sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < OBJ_WAVES; ++w) r += sh[w];
    return r;
}

__device__ __forceinline__ float bce_term(float p, float t) {
    const float lp = fmaxf(logf(p), -100.f), l1 = fmaxf(logf(1.f - p), -100.f);
    return -(t * lp + (1.f - t) * l1);
}

// row k as a target of the batch: its cell's index in out1, or -1 when a coordinate (the sample's among them) is out of range
__device__ __forceinline__ long long target_index(const long long* __restrict__ q, int B, int Cc, int Hh, int Ww) {
    const bool ok = q[0] >= 0 && q[0] < B && q[1] >= 0 && q[1] < Cc && q[2] >= 0 && q[2] < Hh && q[3] >= 0 && q[3] < Ww;
    return ok ? ((q[0] * Cc + q[1]) * Hh + q[2]) * Ww + q[3] : -1;
}

__global__ __launch_bounds__(OBJ_THREADS) void partial_kernel(const float* __restrict__ out1, const long long* __restrict__ coords,
                                                              const float* __restrict__ gains, int K, int B, int Cc, int Hh, int Ww,
                                                              const float* __restrict__ out2, const float* __restrict__ gt,
                                                              long long n_px, int nq, int G, double* __restrict__ per_sample,
                                                              double* __restrict__ part) {
    __shared__ double sh[OBJ_WAVES];
    __shared__ double slot[OBJ_THREADS];
    __shared__ int wave_n[OBJ_WAVES];
    const int b = blockIdx.y, g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (g < G) {
        const float* __restrict__ p = out2 + (size_t)b * n_px;
        const float* __restrict__ t = gt + (size_t)b * n_px;
        const float4* __restrict__ p4 = (const float4*)p;
        const float4* __restrict__ t4 = (const float4*)t;
        double s = 0.0;
        for (int q = g * OBJ_THREADS + tid; q < nq; q += G * OBJ_THREADS) {
            const float4 v = p4[q];
            const float4 w = t4[q];
            s += (double)bce_term(v.x, w.x);
            s += (double)bce_term(v.y, w.y);
            s += (double)bce_term(v.z, w.z);
            s += (double)bce_term(v.w, w.w);
        }
        for (long long i = 4ll * nq + g * OBJ_THREADS + tid; i < n_px; i += G * OBJ_THREADS) s += (double)bce_term(p[i], t[i]);
        s = block_sum(s, sh);
        if (tid == 0) part[(size_t)b * G + g] = s;
        return;
    }
    // the value targets of sample b
    slot[tid] = 0.0;
    int n = 0;                                                      // block-uniform: the sample's rows so far
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += OBJ_THREADS) {
        const int k = k0 + tid;
        bool mine = false;
        float term = 0.f;
        if (k < K) {
            const long long* q = coords + 4 * (size_t)k;
            if (q[0] == (long long)b) {
                const long long at = target_index(q, B, Cc, Hh, Ww);      // the range test precedes the gather
                if (at >= 0) {
                    const float d = out1[at] - gains[k];
                    term = d * d;
                    mine = true;
                }
            }
        }
        const unsigned long long m = __ballot(mine);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int pos = n + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < OBJ_WAVES; ++w) {
            if (w < wave) pos += wave_n[w];
            n += wave_n[w];
        }
        if (mine) slot[pos & (OBJ_THREADS - 1)] += (double)term;
        __syncthreads();
    }
    const double v = block_sum(slot[tid], sh);
    if (tid == 0) {
        per_sample[3 * (size_t)b] = v;
        per_sample[3 * (size_t)b + 1] = (double)n;
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void finish_kernel(const double* __restrict__ part, int G, int B,
                                                             const float* __restrict__ weights, double* __restrict__ per_sample,
                                                             double* __restrict__ totals) {
    __shared__ double sh_v[OBJ_WAVES], sh_o[OBJ_WAVES];
    double sv = 0.0, so = 0.0;
    for (int b = threadIdx.x; b < B; b += OBJ_THREADS) {
        double o = 0.0;
        for (int g = 0; g < G; ++g) o += part[(size_t)b * G + g];
        per_sample[3 * (size_t)b + 2] = o;
        const double w = weights ? (double)weights[b] : 1.0;
        sv += w * per_sample[3 * (size_t)b];
        so += w * o;
    }
    sv = block_sum(sv, sh_v);
    so = block_sum(so, sh_o);
    if (threadIdx.x == 0) {
        totals[0] = sv;
        totals[1] = so;
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void backward_kernel(const float* __restrict__ out1, const long long* __restrict__ coords,
                                                               const float* __restrict__ gains, int K, int B, int Cc, int Hh, int Ww,
                                                               const float* __restrict__ out2, const float* __restrict__ gt,
                                                               long long n_px, int nq, int G, const float* __restrict__ weights,
                                                               const float* __restrict__ coef, float* __restrict__ d_out1,
                                                               float* __restrict__ d_out2) {
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    if (blk < B * G) {
        const int b = blk / G, g = blk - b * G;
        const float w = weights ? weights[b] : 1.f;
        const float inv = coef[1] * w / (float)((long long)B * n_px);
        const float* __restrict__ p = out2 + (size_t)b * n_px;
        const float* __restrict__ t = gt + (size_t)b * n_px;
        float* __restrict__ d = d_out2 + (size_t)b * n_px;
        for (int q = g * OBJ_THREADS + tid; q < nq; q += G * OBJ_THREADS) {
            const float4 v = ((const float4*)p)[q];
            const float4 l = ((const float4*)t)[q];
            float4 r;
            r.x = (v.x - l.x) / fmaxf(v.x * (1.f - v.x), 1e-12f) * inv;
            r.y = (v.y - l.y) / fmaxf(v.y * (1.f - v.y), 1e-12f) * inv;
            r.z = (v.z - l.z) / fmaxf(v.z * (1.f - v.z), 1e-12f) * inv;
            r.w = (v.w - l.w) / fmaxf(v.w * (1.f - v.w), 1e-12f) * inv;
            ((float4*)d)[q] = r;
        }
        for (long long i = 4ll * nq + g * OBJ_THREADS + tid; i < n_px; i += G * OBJ_THREADS)
            d[i] = (p[i] - t[i]) / fmaxf(p[i] * (1.f - p[i]), 1e-12f) * inv;
        return;
    }
    // (only launched with K > 0; d_out1 was zeroed by the fill in front of this launch on the same stream)
    const long long k = (long long)(blk - B * G) * OBJ_THREADS + tid;
    if (k >= K) return;
    const long long* q = coords + 4 * (size_t)k;
    const long long at = target_index(q, B, Cc, Hh, Ww);
    if (at < 0) return;
    const float w = weights ? weights[q[0]] : 1.f;
    const float inv = coef[0] * w / (float)K;
    atomicAdd(&d_out1[at], 2.f * (out1[at] - gains[k]) * inv);
}

// NBP_E_* of the arguments the forward and the backward share, 0 when they are fine
int check_common(const float* out1, const long long* coords, const float* gains, int K, int C, int H, int W, const float* out2,
                 const float* gt, int B, int S, const void* ws, size_t ws_bytes) {
    NBP_RETURN_IF(!out1 || !out2 || !gt || !ws, NBP_E_ARG);
    NBP_RETURN_IF(B < 1 || S < 1 || K < 0 || C < 1 || H < 1 || W < 1, NBP_E_ARG);
    NBP_RETURN_IF(K > 0 && (!coords || !gains), NBP_E_ARG);
    NBP_RETURN_IF(B > 65535 || S > 32768, NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < nbp_objective_workspace_bytes(B, S), NBP_E_WS);
    return 0;
}

}  // namespace

extern "C" size_t nbp_objective_workspace_bytes(int B, int S) {
    if (B < 1 || S < 1) return 0;
    return (size_t)B * obj_wgs(S) * sizeof(double) + 256;
}

extern "C" int nbp_objective_forward_f32(const float* out1_nchw, const long long* coords_bcxy, const float* gains, int K, int C, int H,
                                         int W, const float* out2, const float* gt, int B, int S, const float* weights_or_null,
                                         double* per_sample, double* totals, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!per_sample || !totals, NBP_E_ARG);
    int rc = check_common(out1_nchw, coords_bcxy, gains, K, C, H, W, out2, gt, B, S, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    const int G = obj_wgs(S);
    const int nq = obj_quads(S, out2, gt, nullptr);
    partial_kernel<<<dim3((unsigned)(G + 1), (unsigned)B), OBJ_THREADS, 0, st>>>(out1_nchw, coords_bcxy, gains, K, B, C, H, W, out2, gt,
                                                                                 (long long)S * S, nq, G, per_sample, part);
    if ((rc = nbp_launch_status())) return rc;
    finish_kernel<<<1, OBJ_THREADS, 0, st>>>(part, G, B, weights_or_null, per_sample, totals);
    return nbp_launch_status();
}

extern "C" int nbp_objective_backward_f32(const float* out1_nchw, const long long* coords_bcxy, const float* gains, int K, int C,
                                          int H, int W, const float* out2, const float* gt, int B, int S,
                                          const float* weights_or_null, const float* coef_dev, float* d_out1_nchw, float* d_out2,
                                          void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!coef_dev || !d_out1_nchw || !d_out2, NBP_E_ARG);
    int rc = check_common(out1_nchw, coords_bcxy, gains, K, C, H, W, out2, gt, B, S, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_out1_nchw, 0, (size_t)B * C * H * W * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    const int G = obj_wgs(S);
    const int nq = obj_quads(S, out2, gt, d_out2);
    const long long blocks = (long long)B * G + nbp_cdiv(K, OBJ_THREADS);
    backward_kernel<<<(unsigned)blocks, OBJ_THREADS, 0, st>>>(out1_nchw, coords_bcxy, gains, K, B, C, H, W, out2, gt, (long long)S * S,
                                                              nq, G, weights_or_null, coef_dev, d_out1_nchw, d_out2);
    return nbp_launch_status();
}
