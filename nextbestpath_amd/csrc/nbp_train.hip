// nbp_train.hip -- kernels of the NBP training step (forward in train mode + backward), fp32.
//
// Replaces what autograd + cuDNN/MIOpen execute under
// next_best_path/utility/nbp_utils.py:340-395 (train_experience_data: nbp.train(); forward;
// gather pred[b,c,x,y]; NBP.loss; backward) for the layers of
// next_best_path/networks/nbp_model.py:8-62:
//   * conv weight gradient on the matrix cores (wgrad: reduction over pixels);
//     the data gradient reuses the forward implicit-GEMM kernel with flipped/transposed weights
//   * BatchNorm2d in training mode: batch statistics, running-stat update, backward
//   * MaxPool2d backward, nearest-upsample backward (2x2 sum), attention-gate pieces,
//     sparse value-map loss gather / scatter, BCE
// Activations are NHWC [M, C] with M = B*H*W.  Reductions are two-stage (per-workgroup partials,
// then a finalize kernel) so results are run-to-run deterministic.
#include "common.h"
#include <cstdlib>

namespace {

// ------------------------------------------------------------------ column reductions over [M, C]
// MODE 0: out0[c] = sum x           out1[c] = sum x*x
// MODE 1: out0[c] = sum dz          out1[c] = sum dz * xhat,  dz = dy * (y > 0 if relu), xhat = (x-mean)*invstd
// MODE 2: out0[c] = sum s[m]*x[m][c]                         (row-weighted column sum; s may be null = 1)
template <int MODE>
__global__ __launch_bounds__(256) void colreduce_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ y, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const float* __restrict__ rows,
                                                        long long M, int C, int relu, long long rows_per_block,
                                                        double* __restrict__ part) {
    // thread t owns channel c = t % CT (CT = min(C,256) rounded), and rows r = t / CT + k * (256 / CT).
    // Sums are carried in DOUBLE from the first add to the per-block partial (torch's CPU BatchNorm accumulates in double
    // too): the backward combines them as dz - mean(dz) - xhat mean(dz xhat), which cancels to 1e-4 of |dz| over the
    // constant background of a count map -- fp32 partial sums left 1e-2 relative error in the encoder gradients.
    const int CT = C < 256 ? C : 256;
    const int rpb = 256 / CT;                         // rows processed per pass
    const int c_local = threadIdx.x % CT, rsub = threadIdx.x / CT;
    __shared__ double sh0[256], sh1[256];
    for (int c0 = 0; c0 < C; c0 += CT) {
        const int c = c0 + c_local;
        double s0 = 0.0, s1 = 0.0;
        if (rsub < rpb && c < C) {
            const long long r_begin = (long long)blockIdx.x * rows_per_block;
            const long long r_end = r_begin + rows_per_block < M ? r_begin + rows_per_block : M;
            float mu = 0.f, is = 0.f;
            if (MODE == 1) { mu = mean[c]; is = invstd[c]; }
            if (MODE == 0) mu = a[c];          // shift = the first row: sums of (x - k), (x - k)^2 do not cancel when |mean| >> std
            for (long long r = r_begin + rsub; r < r_end; r += rpb) {
                const float v = a[r * C + c];
                if (MODE == 0) { const double d = (double)v - (double)mu; s0 += d; s1 += d * d; }
                if (MODE == 1) {
                    float dz = v;                                   // a = dy
                    if (relu && !(y[r * C + c] > 0.f)) dz = 0.f;
                    s0 += (double)dz; s1 += (double)dz * (((double)b[r * C + c] - (double)mu) * (double)is); // b = x
                }
                if (MODE == 2) s0 += (double)(rows ? rows[r] : 1.f) * (double)v;
            }
        }
        sh0[threadIdx.x] = s0; sh1[threadIdx.x] = s1;
        __syncthreads();
        if (rsub == 0 && c < C) {
            for (int k = 1; k < rpb; ++k) { s0 += sh0[k * CT + c_local]; s1 += sh1[k * CT + c_local]; }
            part[((long long)blockIdx.x * 2 + 0) * C + c] = s0;
            part[((long long)blockIdx.x * 2 + 1) * C + c] = s1;
        }
        __syncthreads();
    }
}

// Same reduction for C % 4 == 0 with 16-B loads: thread t owns four channels (float4 column t % CT) and the rows
// rsub + k * rpb of its block, four rows in flight per iteration.  The scalar kernel above keeps C = 1 (psi BatchNorm).
typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f64x4 to_d4(f32x4 v) { return f64x4{(double)v[0], (double)v[1], (double)v[2], (double)v[3]}; }

// The train-mode BatchNorm output of four channels, evaluated in double from the UNROUNDED statistics and rounded once
// (bn_apply4_kernel).  The backward kernels call the same function on the same inputs to rebuild the ReLU mask (y > 0) from x,
// which they read anyway, instead of reading y: two of the ten tensor passes a BatchNorm costs per step (round 4).
// The forward (bn_apply4_kernel) and three backward kernels must round IDENTICALLY for the rebuilt mask to be the forward's: the
// expression is evaluated without contraction -- sub, mul, mul, add, each rounded -- whatever the surrounding kernel's code looks
// like to the optimiser (left to the compiler, an fma in one kernel and not in another would flip masks at y = 0).
__device__ __forceinline__ f32x4 bn_value4(f32x4 x, f64x4 mu, f64x4 is, f64x4 g, f64x4 bt) {
#pragma clang fp contract(off)
    const f64x4 d = to_d4(x) - mu;
    const f64x4 n = d * is;
    const f64x4 s = n * g;
    const f64x4 r = s + bt;
    return f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
}
// stat_d = [mean | invstd | lo | hi] doubles (nbp_bn_train_forward_stat4_f32), or null: mask from y.
// lo / hi: bn_value is a composition of rounded monotone operations, hence monotone in x (direction = sign of gamma), so the
// forward's ReLU mask (y > 0) is EXACTLY lo <= x <= hi for two floats found once per channel by bisection over the ordered floats
// with the forward's own arithmetic (bn_finalize_kernel).  The backward kernels test two fp32 compares per element instead of
// re-evaluating six double-precision operations: they were co-limited by the fp64 pipe (3.0 - 3.8 TB/s; round 5).
struct MaskStat { const double* stat_d; const float* gamma; const float* beta; };
__device__ __forceinline__ float bn_value1(float x, double mu, double is, double g, double bt) {      // bn_value4, one element
#pragma clang fp contract(off)
    const double d = (double)x - mu;
    const double n = d * is;
    const double s = n * g;
    const double r = s + bt;
    return (float)r;
}
// order-preserving map between non-NaN floats and signed integers (its own inverse)
__device__ __forceinline__ int float_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }
// lo <= x <= hi  <=>  bn_value1(x) > 0, for finite x
__device__ inline void bn_mask_bounds(double mu, double is, double g, double bt, float* lo_out, float* hi_out) {
    const float INF = __int_as_float(0x7f800000), FMAX = __int_as_float(0x7f7fffff);
    auto P = [&](int key) { return bn_value1(__int_as_float(float_key(key)), mu, is, g, bt) > 0.f; };
    const int kmin = float_key(__float_as_int(-FMAX)), kmax = float_key(__float_as_int(FMAX));
    float lo = INF, hi = -INF;                               // never
    if (!(g > 0.0) && !(g < 0.0)) {                          // gamma == 0 (or NaN): y = beta for every finite x
        if (P(float_key(0))) { lo = -INF; hi = INF; }
    } else if (g > 0.0) {                                    // increasing: the smallest x with y > 0
        if (P(kmin)) { lo = -INF; hi = INF; }
        else if (P(kmax)) {
            long long a = kmin, b = kmax;                    // P(a) false, P(b) true
            while (b - a > 1) { const long long m = a + (b - a) / 2; if (P((int)m)) b = m; else a = m; }
            lo = __int_as_float(float_key((int)b)); hi = INF;
        }
    } else {                                                 // decreasing: the largest x with y > 0
        if (P(kmax)) { lo = -INF; hi = INF; }
        else if (P(kmin)) {
            long long a = kmin, b = kmax;                    // P(a) true, P(b) false
            while (b - a > 1) { const long long m = a + (b - a) / 2; if (P((int)m)) a = m; else b = m; }
            lo = -INF; hi = __int_as_float(float_key((int)a));
        }
    }
    *lo_out = lo; *hi_out = hi;
}

template <int MODE>
__global__ __launch_bounds__(256) void colreduce4_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ y, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, const float* __restrict__ rows,
                                                         long long M, int C4, int relu, long long rows_per_block,
                                                         double* __restrict__ part, MaskStat ms = MaskStat{nullptr, nullptr, nullptr}) {
    const int CT = C4 < 256 ? C4 : 256;
    const int rpb = 256 / CT;
    const int c_local = threadIdx.x % CT, rsub = threadIdx.x / CT;
    __shared__ f64x4 sh0[256], sh1[256];
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y);
    // Rows are dealt to the workgroups in CHUNKS of 4 rpb rows, chunk k to workgroup k mod gridDim.x (round 5): with one contiguous
    // run of rows per workgroup all 1024 workgroups walked their runs in step, 512 KB apart on the large tensors -- the same few HBM
    // channels at any moment (3.0 - 3.5 TB/s); interleaved 16-KB chunks spread every moment's requests over all channels.
    (void)rows_per_block;
    const long long R = 4ll * rpb, n_chunks = (M + R - 1) / R;
    for (int c0 = 0; c0 < C4; c0 += CT) {
        const int c = c0 + c_local;
        f64x4 s0 = {0.0, 0.0, 0.0, 0.0}, s1 = {0.0, 0.0, 0.0, 0.0};
        if (rsub < rpb && c < C4) {
            f64x4 mu = {0.0, 0.0, 0.0, 0.0};
            if (MODE == 0) mu = to_d4(a4[c]);  // shift = the first row (see colreduce_kernel)
            // MODE 1, mask from the statistics: two fp32 bounds per channel (MaskStat)
            const bool stat_mask = MODE == 1 && relu && ms.stat_d;
            f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
            if (stat_mask) {
                const f64x4 l = reinterpret_cast<const f64x4*>(ms.stat_d + 8 * (size_t)C4)[c], h = reinterpret_cast<const f64x4*>(ms.stat_d + 12 * (size_t)C4)[c];
                lo = f32x4{(float)l[0], (float)l[1], (float)l[2], (float)l[3]}; hi = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            }
            auto step = [&](long long r) {
                const f32x4 v = a4[r * C4 + c];
                if (MODE == 0) { const f64x4 d = to_d4(v) - mu; s0 += d; s1 += d * d; }
                if (MODE == 1) {
                    // s1 = sum dz x (RAW: the finalizer turns it into sum dz xhat = invstd (s1 - mean s0), in double): two
                    // double operations per element here instead of five
                    f32x4 dz = v;
                    const f32x4 xv = b4[r * C4 + c];
                    if (relu) {
                        if (stat_mask) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (!(xv[e] >= lo[e] && xv[e] <= hi[e])) dz[e] = 0.f;
                        } else {
                            const f32x4 yy = y4[r * C4 + c];
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (!(yy[e] > 0.f)) dz[e] = 0.f;
                        }
                    }
                    const f64x4 dzd = to_d4(dz);
                    s0 += dzd; s1 += dzd * to_d4(xv);
                }
                if (MODE == 2) s0 += to_d4(v) * (double)(rows ? rows[r] : 1.f);
            };
            for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
                const long long r = ch * R + rsub;
                if (r + 3 * rpb < M) { step(r); step(r + rpb); step(r + 2 * rpb); step(r + 3 * rpb); }
                else
                    for (long long q = r; q < M; q += rpb) step(q);
            }
        }
        sh0[threadIdx.x] = s0; sh1[threadIdx.x] = s1;
        __syncthreads();
        if (rsub == 0 && c < C4) {
            for (int k = 1; k < rpb; ++k) { s0 += sh0[k * CT + c_local]; s1 += sh1[k * CT + c_local]; }
            reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 0) * C4 * 4)[c] = s0;
            reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 1) * C4 * 4)[c] = s1;
        }
        __syncthreads();
    }
}

// Column sums of the per-block partials part[k][2][C]: a 256-thread block owns FIN_CH = 8 channels; thread (c, ks) adds the
// rows k = ks, ks + 32, ... in double (fixed order, four loads in flight), the 32 slices meet in LDS in a fixed order:
// deterministic, and nblk / 32 dependent loads per thread.  (Round 3 had 32 channels x 8 slices: with 64 channels that was a
// grid of TWO workgroups walking 128-long chains -- 14 us per finalize, ~150 of them per training step.)
constexpr int FIN_CH = 8, FIN_SL = 256 / FIN_CH;
__device__ __forceinline__ void colsum_pair(const double* __restrict__ part, int nblk, int C, int c, int ks, double (*sh)[2][FIN_CH],
                                            double* s0_out, double* s1_out) {
    double s0 = 0, s1 = 0;
    if (c < C) {
        int k = ks;
        for (; k + 3 * FIN_SL < nblk; k += 4 * FIN_SL) {          // four rows in flight, added in the same order as one at a time
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = part[((long long)(k + FIN_SL * u) * 2) * C + c]; b[u] = part[((long long)(k + FIN_SL * u) * 2 + 1) * C + c]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s0 += a[u]; s1 += b[u]; }
        }
        for (; k < nblk; k += FIN_SL) { s0 += part[((long long)k * 2) * C + c]; s1 += part[((long long)k * 2 + 1) * C + c]; }
    }
    sh[ks][0][threadIdx.x % FIN_CH] = s0; sh[ks][1][threadIdx.x % FIN_CH] = s1;
    __syncthreads();
    s0 = 0; s1 = 0;
    if (ks == 0)
        for (int q = 0; q < FIN_SL; ++q) { s0 += sh[q][0][threadIdx.x % FIN_CH]; s1 += sh[q][1][threadIdx.x % FIN_CH]; }
    *s0_out = s0; *s1_out = s1;
}

// finalize MODE 0 (partials are sums of (x - k), (x - k)^2 with k = x[0][c]): mean = k + s0/M, biased var = s1/M - (s0/M)^2
// -> invstd; running stats (momentum, unbiased var).  Shifted sums: fp32 partials lose ~1e-7 (1 + ((mean-k)/std)^2) of
// the variance instead of 1e-7 mean^2/var (torch uses Welford).
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ x_first_row,
                                                          const double* __restrict__ part, int nblk, int C, long long M, float eps,
                                                          float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                          float* __restrict__ run_mean, float* __restrict__ run_var,
                                                          double* __restrict__ stat_d, const float* __restrict__ gamma = nullptr,
                                                          const float* __restrict__ beta = nullptr, int four_planes = 0) {
    __shared__ double sh[FIN_SL][2][FIN_CH];
    const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH, ks = threadIdx.x / FIN_CH;
    double s0, s1;
    colsum_pair(part, nblk, C, c, ks, sh, &s0, &s1);
    if (c >= C || ks != 0) return;
    const double dm = s0 / (double)M;
    const double mu = (double)x_first_row[c] + dm;
    double var = s1 / (double)M - dm * dm;
    if (var < 0) var = 0;
    mean[c] = (float)mu;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    stat_d[c] = mu; stat_d[C + c] = 1.0 / sqrt(var + (double)eps);      // unrounded, for the forward normalisation
    if (gamma) {                // the ReLU mask of this channel as two float bounds (MaskStat): [2C, 3C) lo, [3C, 4C) hi
        float lo, hi;
        bn_mask_bounds(mu, 1.0 / sqrt(var + (double)eps), (double)gamma[c], (double)beta[c], &lo, &hi);
        stat_d[2 * C + c] = (double)lo; stat_d[3 * C + c] = (double)hi;
    } else if (four_planes) {   // no ReLU in this forward: "every element passes"
        stat_d[2 * C + c] = (double)__int_as_float(0xff800000); stat_d[3 * C + c] = (double)__int_as_float(0x7f800000);
    }
    if (run_mean) {
        const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
        run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mu);
        run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
    }
}

// finalize generic: out0[c] (+ out1[c]) = sum over blocks
// raw_mean / raw_invstd (not null): the second sum is sum dz x (colreduce4_kernel<1>) and becomes sum dz xhat here
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const double* __restrict__ part, int nblk, int C,
                                                              float* __restrict__ out0, float* __restrict__ out1,
                                                              double* __restrict__ out_d = nullptr,
                                                              const float* __restrict__ raw_mean = nullptr,
                                                              const float* __restrict__ raw_invstd = nullptr) {
    __shared__ double sh[FIN_SL][2][FIN_CH];
    const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH, ks = threadIdx.x / FIN_CH;
    double s0, s1;
    colsum_pair(part, nblk, C, c, ks, sh, &s0, &s1);
    if (c >= C || ks != 0) return;
    if (raw_mean) s1 = (double)raw_invstd[c] * (s1 - (double)raw_mean[c] * s0);
    if (out0) out0[c] = (float)s0;
    if (out1) out1[c] = (float)s1;
    if (out_d) { out_d[c] = s0; out_d[C + c] = s1; }          // unrounded sums for the backward apply
}

// y = (x - mean) invstd gamma + beta evaluated per element in double from the unrounded statistics and rounded once: the
// forward noise decides how many ReLU masks flip against an exact evaluation (each flip moves a gradient tensor by ~1e-4).
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long long total, int C,
                                                       const double* __restrict__ stat_d,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       int relu, float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        float v = (float)(((double)x[i] - stat_d[c]) * stat_d[C + c] * (double)gamma[c] + (double)beta[c]);
        if (relu) v = fmaxf(v, 0.f);
        y[i] = v;
    }
}

// dx = gamma*invstd/M * (M*dz - dbeta - xhat*dgamma), evaluated per element in double from the unrounded sums (sums[0..C) =
// dbeta, sums[C..2C) = dgamma) and rounded once, like torch's CPU kernel (accscalar_t = double): the bracket cancels.
__global__ __launch_bounds__(256) void bn_backward_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ y, long long total, int C,
                                                                long long M, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma,
                                                                const double* __restrict__ sums, int relu,
                                                                float* __restrict__ dx) {
    const double invM = 1.0 / (double)M;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        float dz = dy[i];
        if (relu && !(y[i] > 0.f)) dz = 0.f;
        const double is = (double)invstd[c];
        const double xhat = ((double)x[i] - (double)mean[c]) * is;
        dx[i] = (float)((double)gamma[c] * is * ((double)dz - invM * (sums[c] + xhat * sums[C + c])));
    }
}

// max |.| of a tensor for the split convolutions' operand scale (nbp_split.hip): float bits, atomicMax spread over 64 words
__device__ __forceinline__ void train_wave_amax(float mx, unsigned* out) {
#pragma unroll
    for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & 63u), __float_as_uint(mx));
}

__global__ __launch_bounds__(256) void bn_apply4_kernel(const float* __restrict__ x, long long total4, int C4,
                                                        const double* __restrict__ stat_d,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int relu, float* __restrict__ y, unsigned* __restrict__ amax_out) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    f32x4* y4 = reinterpret_cast<f32x4*>(y);
    const f64x4* mu4 = reinterpret_cast<const f64x4*>(stat_d);
    const f64x4* is4 = reinterpret_cast<const f64x4*>(stat_d + 4 * (size_t)C4);
    float mx = 0.f;
    const long long stride = (long long)gridDim.x * blockDim.x;
    if (256 % C4 == 0) {
        // every channel count of the network: the stride is a multiple of C4, so a thread stays on ONE float4 column -- its four
        // channels' statistics are loaded once (per element they were 96 B of cached parameters beside 16 B of data), and four
        // rows are in flight per iteration
        const int c = threadIdx.x % C4;
        const f64x4 mu = mu4[c], is = is4[c];
        const f64x4 g = to_d4(reinterpret_cast<const f32x4*>(gamma)[c]), bt = to_d4(reinterpret_cast<const f32x4*>(beta)[c]);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += 4 * stride) {
            f32x4 xv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (i + k * stride < total4) xv[k] = x4[i + k * stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k * stride >= total4) break;
                f32x4 v = bn_value4(xv[k], mu, is, g, bt);
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                y4[i + k * stride] = v;
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
            }
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += stride) {
            const int c = (int)(i % C4);
            const f64x4 g = to_d4(reinterpret_cast<const f32x4*>(gamma)[c]), bt = to_d4(reinterpret_cast<const f32x4*>(beta)[c]);
            f32x4 v = bn_value4(x4[i], mu4[c], is4[c], g, bt);
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            y4[i] = v;
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
    }
    if (amax_out) train_wave_amax(mx, amax_out);
}

// dx = gamma invstd (dz - (dbeta + xhat dgamma) / M) as an AFFINE form per channel, dx = A dz + (B x + D) with
//   A = gamma invstd,  B = -A invstd dgamma / M,  D = -A (dbeta - mean invstd dgamma) / M
// evaluated in double and rounded once: two fused multiply-adds per element instead of six double operations (the large terms
// B x and D cancel to ~|mean| / std of their size: 1e-16 relative of that in double).  The ReLU mask comes from the two float
// bounds of MaskStat (or from y).
struct BnAffine { f64x4 A, B, D; f32x4 lo, hi; };
__device__ __forceinline__ BnAffine bn_affine4(int c, int C4, const float* mean, const float* invstd, const float* gamma, const double* sums,
                                               double invM, const MaskStat& ms, bool stat_mask) {
    BnAffine k;
    const f64x4 mu = to_d4(reinterpret_cast<const f32x4*>(mean)[c]), is = to_d4(reinterpret_cast<const f32x4*>(invstd)[c]);
    const f64x4 g = to_d4(reinterpret_cast<const f32x4*>(gamma)[c]);
    const f64x4 kb = reinterpret_cast<const f64x4*>(sums)[c], kg = reinterpret_cast<const f64x4*>(sums + 4 * (size_t)C4)[c];
    k.A = g * is;
    k.B = -(k.A * is * kg) * invM;
    k.D = -(k.A * (kb - mu * is * kg)) * invM;
    k.lo = f32x4{0.f, 0.f, 0.f, 0.f}; k.hi = k.lo;
    if (stat_mask) {
        const f64x4 l = reinterpret_cast<const f64x4*>(ms.stat_d + 8 * (size_t)C4)[c], h = reinterpret_cast<const f64x4*>(ms.stat_d + 12 * (size_t)C4)[c];
        k.lo = f32x4{(float)l[0], (float)l[1], (float)l[2], (float)l[3]}; k.hi = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    return k;
}
__device__ __forceinline__ f32x4 bn_dx4(f32x4 dz, f32x4 xv, f32x4 yy, const BnAffine& k, int relu, bool stat_mask) {
    if (relu) {
        if (stat_mask) {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (!(xv[e] >= k.lo[e] && xv[e] <= k.hi[e])) dz[e] = 0.f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (!(yy[e] > 0.f)) dz[e] = 0.f;
        }
    }
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)fma(k.A[e], (double)dz[e], fma(k.B[e], (double)xv[e], k.D[e]));
    return o;
}

__global__ __launch_bounds__(256) void bn_backward_apply4_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ y, long long total4, int C4,
                                                                 long long M, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma,
                                                                 const double* __restrict__ sums, int relu,
                                                                 float* __restrict__ dx, MaskStat ms) {
    const double invM = 1.0 / (double)M;
    const f32x4* dy4 = reinterpret_cast<const f32x4*>(dy);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y);
    f32x4* dx4 = reinterpret_cast<f32x4*>(dx);
    const bool stat_mask = relu && ms.stat_d;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const BnAffine k = bn_affine4(c, C4, mean, invstd, gamma, sums, invM, ms, stat_mask);
        const f32x4 xv = x4[i];
        dx4[i] = bn_dx4(dy4[i], xv, (relu && !stat_mask) ? y4[i] : xv, k, relu, stat_mask);
    }
}

// The same with the consumers' passes folded in: the convolution in front of this BatchNorm needs sum_m dx[m][c] (its bias
// gradient) and max |dx| (the split scheme's scale of its data / weight gradients) -- two more reads of dx as separate kernels.
// Thread layout of colreduce4_kernel (a thread owns one float4 column and the rows rsub + k rpb of its block, four rows in flight),
// the column sums of the ROUNDED dx in double, per-block partials [block][2][C] for colsum_finalize_kernel.
__global__ __launch_bounds__(256) void bn_backward_apply4_sum_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                     const float* __restrict__ y, long long M, int C4,
                                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                     const float* __restrict__ gamma, const double* __restrict__ sums,
                                                                     int relu, long long rows_per_block, float* __restrict__ dx,
                                                                     double* __restrict__ part, unsigned* __restrict__ amax_out, MaskStat ms) {
    const int CT = C4 < 256 ? C4 : 256;
    const int rpb = 256 / CT;
    const int c_local = threadIdx.x % CT, rsub = threadIdx.x / CT;
    __shared__ f64x4 sh0[256];
    const double invM = 1.0 / (double)M;
    const f32x4* dy4 = reinterpret_cast<const f32x4*>(dy);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y);
    f32x4* dx4 = reinterpret_cast<f32x4*>(dx);
    (void)rows_per_block;                      // chunks of 4 rpb rows, chunk k to workgroup k mod gridDim.x (see colreduce4_kernel)
    const long long R = 4ll * rpb, n_chunks = (M + R - 1) / R;
    const bool stat_mask = relu && ms.stat_d;
    const bool from_y = relu && !stat_mask;
    float mx = 0.f;
    for (int c0 = 0; c0 < C4; c0 += CT) {
        const int c = c0 + c_local;
        f64x4 s0 = {0.0, 0.0, 0.0, 0.0};
        if (rsub < rpb && c < C4) {
            const BnAffine k = bn_affine4(c, C4, mean, invstd, gamma, sums, invM, ms, stat_mask);
            auto emit = [&](long long i, f32x4 dz, f32x4 xv, f32x4 yy) {
                const f32x4 o = bn_dx4(dz, xv, yy, k, relu, stat_mask);
                dx4[i] = o;
                s0 += to_d4(o);
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
            };
            for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
                const long long r = ch * R + rsub;
                if (r + 3 * rpb < M) {                           // four rows in flight (8 - 12 loads), the sums in row order
                    f32x4 dz[4], xv[4], yy[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const long long i = (r + u * rpb) * C4 + c;
                        dz[u] = dy4[i]; xv[u] = x4[i]; yy[u] = from_y ? y4[i] : xv[u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) emit((r + u * rpb) * C4 + c, dz[u], xv[u], yy[u]);
                } else {
                    for (long long q = r; q < M; q += rpb) {
                        const long long i = q * C4 + c;
                        const f32x4 xv = x4[i];
                        emit(i, dy4[i], xv, from_y ? y4[i] : xv);
                    }
                }
            }
        }
        sh0[threadIdx.x] = s0;
        __syncthreads();
        if (rsub == 0 && c < C4) {
            for (int k = 1; k < rpb; ++k) s0 += sh0[k * CT + c_local];
            reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 0) * C4 * 4)[c] = s0;
            reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 1) * C4 * 4)[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
    }
    if (amax_out) train_wave_amax(mx, amax_out);
}

// ------------------------------------------------------------------ the attention gate's element-wise middle, fused (round 6)
// Attention_block.forward (nbp_model.py:52-60) between the two 1x1 convolutions and x * psi:
//     g1 = BN_g(g_pre);  x1 = BN_x(x_pre);  q = relu(g1 + x1);  p = psi_conv(q) = q . w + b
// as its own launches these were BN apply (R + W) twice, add-relu (2 R + W), row-dot (R) over [M, F_int] tensors -- 8 passes; here
// ONE pass reads g_pre and x_pre, writes q and p (3 passes).  g1 and x1 are evaluated exactly as bn_apply4_kernel does (bn_value4,
// rounded to fp32 each) and p sums its row in rowdot_kernel's order: q and p are the separate launches' bit for bit.  Thread layout: a thread owns one float4 column (256 % F4 == 0) and walks rows; the F4 lanes of
// a row are consecutive lanes of one wave.
struct GateBn { const double* stat_g; const double* stat_x; const float* gamma_g; const float* beta_g; const float* gamma_x; const float* beta_x; };
__global__ __launch_bounds__(256) void gate_mid_fwd4_kernel(const float* __restrict__ gp, const float* __restrict__ xp, long long M, int F4,
                                                            GateBn bn, const float* __restrict__ w, const float* __restrict__ b,
                                                            float* __restrict__ q, float* __restrict__ p) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gp);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xp);
    f32x4* q4 = reinterpret_cast<f32x4*>(q);
    const int c = threadIdx.x % F4, rsub = threadIdx.x / F4, rpb = 256 / F4;
    const f64x4 mug = reinterpret_cast<const f64x4*>(bn.stat_g)[c], isg = reinterpret_cast<const f64x4*>(bn.stat_g + 4 * (size_t)F4)[c];
    const f64x4 mux = reinterpret_cast<const f64x4*>(bn.stat_x)[c], isx = reinterpret_cast<const f64x4*>(bn.stat_x + 4 * (size_t)F4)[c];
    const f64x4 gg = to_d4(reinterpret_cast<const f32x4*>(bn.gamma_g)[c]), bg = to_d4(reinterpret_cast<const f32x4*>(bn.beta_g)[c]);
    const f64x4 gx = to_d4(reinterpret_cast<const f32x4*>(bn.gamma_x)[c]), bx = to_d4(reinterpret_cast<const f32x4*>(bn.beta_x)[c]);
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[c];
    const float b0 = b[0];
    const long long rstep = (long long)gridDim.x * rpb;
    // (every lane of a row's group runs the same trip count: the shuffles below need the whole group)
    for (long long r0 = (long long)blockIdx.x * rpb; r0 < M; r0 += 2 * rstep) {
        f32x4 gv[2], xv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long long r = r0 + u * rstep + rsub;
            if (r < M) { gv[u] = g4[r * F4 + c]; xv[u] = x4[r * F4 + c]; }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long long r = r0 + u * rstep + rsub;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (r < M) {
                const f32x4 a = bn_value4(gv[u], mug, isg, gg, bg), t = bn_value4(xv[u], mux, isx, gx, bx);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fmaxf(a[e] + t[e], 0.f);
                q4[r * F4 + c] = o;
            }
            // p = q . w in rowdot_kernel's order, so that p -- and with it everything downstream -- is the separate launches' bit for bit:
            // there, lane L of 16 chains fmaf over the elements L, L + 16, L + 32, ... and the 16 chains meet in a xor tree 8, 4, 2, 1.
            // Element e of this lane's float4 (column c) is element 4 c + e of the row: chain L = 4 (c & 3) + e, position c >> 2.  The
            // chains run down the lanes c, c + 4, c + 8, ... (F4 / 4 sequential steps), the tree is two lane exchanges and two in-lane adds.
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < (F4 >> 2); ++k) {
                f32x4 prev;
#pragma unroll
                for (int e = 0; e < 4; ++e) prev[e] = __shfl_up(acc[e], 4);
                if ((c >> 2) == k) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(o[e], wv[e], k ? prev[e] : 0.f);
                }
            }
            // (the finished chains sit in the row's last four lanes: L = 4 j + e with j = c & 3)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], 2);         // L ^ 8
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], 1);         // L ^ 4
            const float t0 = acc[0] + acc[2], t1 = acc[1] + acc[3];              // L ^ 2
            if (c == F4 - 1 && r < M) p[r] = (t0 + t1) + b0;                     // L ^ 1, then PsiConvFn's bias add
        }
    }
}

// Backward of the same: from dp (the gradient of p) -- dq = dp (x) w, dz = dq (q > 0) -- both BatchNorm backwards at once.
// Reduce pass: per channel s0 = sum dz, s1g = sum dz g_pre, s1x = sum dz x_pre (raw, as colreduce4_kernel<1>) and sw = sum q dp (the psi
// weight's gradient); rows in colreduce4_kernel's chunk order, so the sums are the separate launches' bit for bit.
__global__ __launch_bounds__(256) void gate_mid_bwd_reduce4_kernel(const float* __restrict__ dp, const float* __restrict__ w,
                                                                   const float* __restrict__ q, const float* __restrict__ gp,
                                                                   const float* __restrict__ xp, long long M, int F4,
                                                                   double* __restrict__ part) {
    const int CT = F4 < 256 ? F4 : 256, rpb = 256 / CT;
    const int c = threadIdx.x % CT, rsub = threadIdx.x / CT;
    __shared__ f64x4 sh[4][256];
    const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gp);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xp);
    const long long R = 4ll * rpb, n_chunks = (M + R - 1) / R;
    f64x4 s0 = {0.0, 0.0, 0.0, 0.0}, s1g = s0, s1x = s0, sw = s0;
    if (rsub < rpb && c < F4) {
        const f32x4 wv = reinterpret_cast<const f32x4*>(w)[c];
        auto step = [&](long long r) {
            const float d = dp[r];
            const f32x4 qv = q4[r * F4 + c], gv = g4[r * F4 + c], xv = x4[r * F4 + c];
            f32x4 dz;
#pragma unroll
            for (int e = 0; e < 4; ++e) dz[e] = qv[e] > 0.f ? d * wv[e] : 0.f;
            const f64x4 dzd = to_d4(dz);
            s0 += dzd; s1g += dzd * to_d4(gv); s1x += dzd * to_d4(xv);
            sw += to_d4(qv) * (double)d;
        };
        for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
            const long long r = ch * R + rsub;
            if (r + 3 * rpb < M) { step(r); step(r + rpb); step(r + 2 * rpb); step(r + 3 * rpb); }
            else
                for (long long k = r; k < M; k += rpb) step(k);
        }
    }
    sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1g; sh[2][threadIdx.x] = s1x; sh[3][threadIdx.x] = sw;
    __syncthreads();
    if (rsub == 0 && c < F4) {
        for (int k = 1; k < rpb; ++k) { s0 += sh[0][k * CT + c]; s1g += sh[1][k * CT + c]; s1x += sh[2][k * CT + c]; sw += sh[3][k * CT + c]; }
        f64x4* o = reinterpret_cast<f64x4*>(part + (long long)blockIdx.x * 4 * F4 * 4);
        o[c] = s0; o[F4 + c] = s1g; o[2 * F4 + c] = s1x; o[3 * F4 + c] = sw;
    }
}

// column sums of the partials [blk][4][C] in the fixed order of colsum_pair (slice ks adds rows ks, ks + 32, ...; the 32 slices meet
// in LDS): dbeta (shared by both BatchNorms) | dgamma_g | dgamma_x | dw_psi, and the unrounded [2 C] sums each apply needs
__global__ __launch_bounds__(256) void gate_mid_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int C,
                                                                    const float* __restrict__ mean_g, const float* __restrict__ invstd_g,
                                                                    const float* __restrict__ mean_x, const float* __restrict__ invstd_x,
                                                                    float* __restrict__ dbeta_g, float* __restrict__ dgamma_g,
                                                                    float* __restrict__ dbeta_x, float* __restrict__ dgamma_x,
                                                                    float* __restrict__ dw, double* __restrict__ sums_g,
                                                                    double* __restrict__ sums_x) {
    __shared__ double sh[FIN_SL][4][FIN_CH];
    const int c = blockIdx.x * FIN_CH + threadIdx.x % FIN_CH, ks = threadIdx.x / FIN_CH;
    double s[4] = {0, 0, 0, 0};
    if (c < C)
        for (int k = ks; k < nblk; k += FIN_SL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += part[((long long)k * 4 + j) * C + c];
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[ks][j][threadIdx.x % FIN_CH] = s[j];
    __syncthreads();
    if (c >= C || ks != 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = 0; for (int k = 0; k < FIN_SL; ++k) s[j] += sh[k][j][threadIdx.x % FIN_CH]; }
    const double dgg = (double)invstd_g[c] * (s[1] - (double)mean_g[c] * s[0]);
    const double dgx = (double)invstd_x[c] * (s[2] - (double)mean_x[c] * s[0]);
    dbeta_g[c] = (float)s[0]; dbeta_x[c] = (float)s[0];
    dgamma_g[c] = (float)dgg; dgamma_x[c] = (float)dgx;
    dw[c] = (float)s[3];
    sums_g[c] = s[0]; sums_g[C + c] = dgg;
    sums_x[c] = s[0]; sums_x[C + c] = dgx;
}

// Apply pass: d g_pre and d x_pre (bn_dx4's affine form, no ReLU inside the BatchNorms), their column sums (the 1x1 convolutions'
// bias gradients) and max |.| (their split data / weight gradients' scale), as bn_backward_apply4_sum_kernel leaves them.
__global__ __launch_bounds__(256) void gate_mid_bwd_apply4_kernel(const float* __restrict__ dp, const float* __restrict__ w,
                                                                  const float* __restrict__ q, const float* __restrict__ gp,
                                                                  const float* __restrict__ xp, long long M, int F4,
                                                                  const float* __restrict__ mean_g, const float* __restrict__ invstd_g,
                                                                  const float* __restrict__ gamma_g, const double* __restrict__ sums_g,
                                                                  const float* __restrict__ mean_x, const float* __restrict__ invstd_x,
                                                                  const float* __restrict__ gamma_x, const double* __restrict__ sums_x,
                                                                  float* __restrict__ dgp, float* __restrict__ dxp,
                                                                  double* __restrict__ part, unsigned* __restrict__ amax_g,
                                                                  unsigned* __restrict__ amax_x) {
    const int CT = F4 < 256 ? F4 : 256, rpb = 256 / CT;
    const int c = threadIdx.x % CT, rsub = threadIdx.x / CT;
    __shared__ f64x4 sh[2][256];
    const double invM = 1.0 / (double)M;
    const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gp);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xp);
    f32x4* dg4 = reinterpret_cast<f32x4*>(dgp);
    f32x4* dx4 = reinterpret_cast<f32x4*>(dxp);
    const long long R = 4ll * rpb, n_chunks = (M + R - 1) / R;
    f64x4 sg = {0.0, 0.0, 0.0, 0.0}, sx = sg;
    float mg = 0.f, mx = 0.f;
    if (rsub < rpb && c < F4) {
        const MaskStat none{nullptr, nullptr, nullptr};
        const BnAffine kg = bn_affine4(c, F4, mean_g, invstd_g, gamma_g, sums_g, invM, none, false);
        const BnAffine kx = bn_affine4(c, F4, mean_x, invstd_x, gamma_x, sums_x, invM, none, false);
        const f32x4 wv = reinterpret_cast<const f32x4*>(w)[c];
        auto emit = [&](long long r, float d, f32x4 qv, f32x4 gv, f32x4 xv) {
            f32x4 dz;
#pragma unroll
            for (int e = 0; e < 4; ++e) dz[e] = qv[e] > 0.f ? d * wv[e] : 0.f;
            const f32x4 og = bn_dx4(dz, gv, gv, kg, 0, false), ox = bn_dx4(dz, xv, xv, kx, 0, false);
            dg4[r * F4 + c] = og; dx4[r * F4 + c] = ox;
            sg += to_d4(og); sx += to_d4(ox);
            mg = fmaxf(fmaxf(mg, fmaxf(fabsf(og[0]), fabsf(og[1]))), fmaxf(fabsf(og[2]), fabsf(og[3])));
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(ox[0]), fabsf(ox[1]))), fmaxf(fabsf(ox[2]), fabsf(ox[3])));
        };
        for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
            const long long r = ch * R + rsub;
            if (r + 3 * rpb < M) {
                float d[4]; f32x4 qv[4], gv[4], xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long i = (r + u * rpb) * F4 + c;
                    d[u] = dp[r + u * rpb]; qv[u] = q4[i]; gv[u] = g4[i]; xv[u] = x4[i];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) emit(r + u * rpb, d[u], qv[u], gv[u], xv[u]);
            } else {
                for (long long k = r; k < M; k += rpb) emit(k, dp[k], q4[k * F4 + c], g4[k * F4 + c], x4[k * F4 + c]);
            }
        }
    }
    sh[0][threadIdx.x] = sg; sh[1][threadIdx.x] = sx;
    __syncthreads();
    if (rsub == 0 && c < F4) {
        for (int k = 1; k < rpb; ++k) { sg += sh[0][k * CT + c]; sx += sh[1][k * CT + c]; }
        reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 0) * F4 * 4)[c] = sg;
        reinterpret_cast<f64x4*>(part + ((long long)blockIdx.x * 2 + 1) * F4 * 4)[c] = sx;
    }
    if (amax_g) train_wave_amax(mg, amax_g);
    if (amax_x) train_wave_amax(mx, amax_x);
}

// ------------------------------------------------------------------ small elementwise pieces
// op 0: out = relu(a + b)          op 1: out = dy * (y > 0)         op 2: out = sigmoid(a)
// op 3: out = dy * y * (1 - y)     op 4: out = a + b                op 5: out = a + b[0]
// sigmoid: 1 / (1 + e^-a) wherever e^-a is finite.  Below a = -88.7 expf(-a) overflows and the quotient was 0 although the value
// (down to e^-103) is an fp32 denormal: there e^a / (1 + e^a), whose numerator is that denormal.
__device__ __forceinline__ float ew_sigmoid(float a) {
    if (a < -88.f) { const float e = expf(a); return e / (1.f + e); }
    return 1.f / (1.f + expf(-a));
}

__global__ __launch_bounds__(256) void ew_kernel(int op, const float* __restrict__ a, const float* __restrict__ b,
                                                 long long n, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v;
        switch (op) {
            case 0: v = fmaxf(a[i] + b[i], 0.f); break;
            case 1: v = b[i] > 0.f ? a[i] : 0.f; break;
            case 2: v = ew_sigmoid(a[i]); break;
            case 3: v = a[i] * b[i] * (1.f - b[i]); break;
            case 5: v = a[i] + b[0]; break;
            default: v = a[i] + b[i]; break;
        }
        out[i] = v;
    }
}

// out[m][c] = x[m][c] * s[m]
__global__ __launch_bounds__(256) void rowscale_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                       long long total, int C, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = x[i] * s[i / C];
}

// 16-B versions of the streaming kernels above / below (sizes and channel counts that are multiples of 4)
__global__ __launch_bounds__(256) void ew4_kernel(int op, const float* __restrict__ a, const float* __restrict__ b,
                                                  long long n4, float* __restrict__ out) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    f32x4* o4 = reinterpret_cast<f32x4*>(out);
    const float b0 = op == 5 ? b[0] : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 x = a4[i];
        f32x4 y = {0.f, 0.f, 0.f, 0.f}, v;
        if (op != 2 && op != 5) y = b4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            switch (op) {
                case 0: v[e] = fmaxf(x[e] + y[e], 0.f); break;
                case 1: v[e] = y[e] > 0.f ? x[e] : 0.f; break;
                case 2: v[e] = ew_sigmoid(x[e]); break;
                case 3: v[e] = x[e] * y[e] * (1.f - y[e]); break;
                case 5: v[e] = x[e] + b0; break;
                default: v[e] = x[e] + y[e]; break;
            }
        }
        o4[i] = v;
    }
}

// out[m][c] = sum_k src_k[m ld_k + c], k = 0 .. n - 1 in that order (fp32, left to right: deterministic): the gradient of a tensor with
// n consumers in ONE pass (n reads, one write) instead of autograd's n - 1 binary adds (3 (n - 1) passes).  A source may be a channel
// slice of a wider tensor (row stride ld_k >= C floats: ConvFn.backward hands out views of a two-source convolution's joint gradient).
constexpr int SUM_N_MAX = 8;
struct SumNArgs { const float* src[SUM_N_MAX]; long long ld4[SUM_N_MAX]; int n; };
__global__ __launch_bounds__(256) void sum_n4_kernel(SumNArgs a, long long M, int C4, float* __restrict__ out) {
    // a thread stays on one float4 column (256 % C4 == 0 for every channel count of the network; wider rows take several columns) and
    // walks rows: no division per element, ROWS rows of every source in flight
    constexpr int ROWS = 2;
    f32x4* o4 = reinterpret_cast<f32x4*>(out);
    const int CT = C4 < 256 ? C4 : 256, rpb = 256 / CT;
    const int c_local = threadIdx.x % CT, rsub = threadIdx.x / CT;
    if (rsub >= rpb) return;
    const long long rstep = (long long)gridDim.x * rpb;
    for (int c = c_local; c < C4; c += CT)
        for (long long r = (long long)blockIdx.x * rpb + rsub; r < M; r += ROWS * rstep) {
            f32x4 v[ROWS][SUM_N_MAX];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const long long ru = r + u * rstep;
                if (ru < M) {
#pragma unroll
                    for (int k = 0; k < SUM_N_MAX; ++k)
                        if (k < a.n) v[u][k] = reinterpret_cast<const f32x4*>(a.src[k])[ru * a.ld4[k] + c];
                }
            }
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const long long ru = r + u * rstep;
                if (ru < M) {
                    f32x4 s = v[u][0];
#pragma unroll
                    for (int k = 1; k < SUM_N_MAX; ++k)
                        if (k < a.n) s += v[u][k];
                    o4[ru * C4 + c] = s;
                }
            }
        }
}

// amax_out (or null): 64 zeroed words that receive max |out| -- the gated tensor feeds a split convolution, whose operand scale would
// otherwise cost a pass of its own over the tensor
__global__ __launch_bounds__(256) void rowscale4_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                        long long total4, int C4, float* __restrict__ out,
                                                        unsigned* __restrict__ amax_out = nullptr) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    f32x4* o4 = reinterpret_cast<f32x4*>(out);
    float mx = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 v = x4[i] * s[i / C4];
        o4[i] = v;
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    if (amax_out) train_wave_amax(mx, amax_out);
}

__global__ __launch_bounds__(256) void slice_channels4_kernel(const float* __restrict__ in, long long M, int Cin4, int c04, int Cs4,
                                                              float* __restrict__ out) {
    const f32x4* i4 = reinterpret_cast<const f32x4*>(in);
    f32x4* o4 = reinterpret_cast<f32x4*>(out);
    const long long total = M * Cs4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        o4[i] = i4[(i / Cs4) * Cin4 + c04 + (i % Cs4)];
}

__global__ __launch_bounds__(256) void sum2x2_4_kernel(const float* __restrict__ dy, int B, int Hs, int Ws, int C4,
                                                       float* __restrict__ out) {
    const f32x4* d4 = reinterpret_cast<const f32x4*>(dy);
    f32x4* o4 = reinterpret_cast<f32x4*>(out);
    const long long total = (long long)B * Hs * Ws * C4;
    const int W = 2 * Ws;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int xs = (int)(p % Ws);
        long long q = p / Ws;
        const int ys = (int)(q % Hs);
        const int b = (int)(q / Hs);
        const long long base = (((long long)b * 2 * Hs + 2 * ys) * W + 2 * xs) * C4 + c;
        o4[i] = (d4[base] + d4[base + C4]) + (d4[base + (long long)W * C4] + d4[base + (long long)W * C4 + C4]);
    }
}

__global__ __launch_bounds__(256) void maxpool2_bwd4_kernel(const float* __restrict__ x, const float* __restrict__ dy, int B,
                                                            int H, int W, int C4, float* __restrict__ dx) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* d4 = reinterpret_cast<const f32x4*>(dy);
    f32x4* o4 = reinterpret_cast<f32x4*>(dx);
    const int Ho = H >> 1, Wo = W >> 1;
    const long long total = (long long)B * Ho * Wo * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long p = i / C4;
        const int xo = (int)(p % Wo);
        long long q = p / Wo;
        const int yo = (int)(q % Ho);
        const int b = (int)(q / Ho);
        const long long base = (((long long)b * H + 2 * yo) * W + 2 * xo) * C4 + c;
        const long long off[4] = {0, C4, (long long)W * C4, (long long)W * C4 + C4};
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x4[base + off[k]];
        const f32x4 g = d4[i];
        f32x4 o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float best = v[0][e];
            int arg = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][e] > best || v[k][e] != v[k][e]) { best = v[k][e]; arg = k; }
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k][e] = k == arg ? g[e] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) o4[base + off[k]] = o[k];
    }
}

// out[m] = sum_c a[m][c] * b[m][c]   (b may be a [C] vector when b_is_vec): 16 lanes per row
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ a, const float* __restrict__ b, int b_is_vec,
                                                     long long M, int C, float* __restrict__ out) {
    const int sub = threadIdx.x & 15;
    const long long rpb = blockDim.x >> 4;
    for (long long m = (long long)blockIdx.x * rpb + (threadIdx.x >> 4); m < M; m += (long long)gridDim.x * rpb) {
        float acc = 0.f;
        for (int c = sub; c < C; c += 16) acc = fmaf(a[m * C + c], b_is_vec ? b[c] : b[m * C + c], acc);
        acc += __shfl_xor(acc, 8, 16);
        acc += __shfl_xor(acc, 4, 16);
        acc += __shfl_xor(acc, 2, 16);
        acc += __shfl_xor(acc, 1, 16);
        if (sub == 0) out[m] = acc;
    }
}

// The backward of out = x * s[m] in ONE pass over dy: dx[m][c] = dy[m][c] * s[m] and ds[m] = sum_c dy[m][c] * x[m][c] (it was a
// row-scale launch plus a row-dot launch, each reading dy).  dy's rows may be ldy >= C floats apart: the gradient of the first
// source of a two-source convolution is a channel slice of the joint gradient, read in place instead of copied out.
// 16 lanes per row, one float4 per lane and step.
__global__ __launch_bounds__(256) void rowscale_bwd4_kernel(const float* __restrict__ dy, long long ldy4, const float* __restrict__ x,
                                                            const float* __restrict__ s, long long M, int C4,
                                                            float* __restrict__ dx, float* __restrict__ ds) {
    const f32x4* dy4 = reinterpret_cast<const f32x4*>(dy);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    f32x4* dx4 = reinterpret_cast<f32x4*>(dx);
    const int sub = threadIdx.x & 15;
    const long long rpb = blockDim.x >> 4;
    for (long long m = (long long)blockIdx.x * rpb + (threadIdx.x >> 4); m < M; m += (long long)gridDim.x * rpb) {
        const float sm = s[m];
        float acc = 0.f;
        for (int c = sub; c < C4; c += 16) {
            const f32x4 g = dy4[m * ldy4 + c], xv = x4[m * C4 + c];
            dx4[m * C4 + c] = g * sm;
            acc = fmaf(g[0], xv[0], acc); acc = fmaf(g[1], xv[1], acc); acc = fmaf(g[2], xv[2], acc); acc = fmaf(g[3], xv[3], acc);
        }
        acc += __shfl_xor(acc, 8, 16);
        acc += __shfl_xor(acc, 4, 16);
        acc += __shfl_xor(acc, 2, 16);
        acc += __shfl_xor(acc, 1, 16);
        if (sub == 0) ds[m] = acc;
    }
}

// out[m][c] = s[m] * w[c]
__global__ __launch_bounds__(256) void outer_kernel(const float* __restrict__ s, const float* __restrict__ w, long long total,
                                                    int C, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = s[i / C] * w[i % C];
}

// MaxPool2d(2,2) backward: the gradient goes to the FIRST maximum of the window in (dy,dx) scan order (ATen rule).
// A NaN takes over from whatever came before it, another NaN included (ATen: val > max || isnan(val)): the LAST NaN of a window wins.
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int B,
                                                           int H, int W, int C, float* __restrict__ dx) {
    const int Ho = H >> 1, Wo = W >> 1;
    const long long total = (long long)B * Ho * Wo * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long p = i / C;
        const int xo = (int)(p % Wo);
        long long q = p / Wo;
        const int yo = (int)(q % Ho);
        const int b = (int)(q / Ho);
        const long long base = (((long long)b * H + 2 * yo) * W + 2 * xo) * C + c;
        const long long off[4] = {0, C, (long long)W * C, (long long)W * C + C};
        float best = x[base];
        int arg = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = x[base + off[k]];
            if (v > best || v != v) { best = v; arg = k; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dx[base + off[k]] = k == arg ? dy[i] : 0.f;
    }
}

// nearest x2 upsample backward: out[b][y][x][c] = sum of the 2x2 block of dy
__global__ __launch_bounds__(256) void sum2x2_kernel(const float* __restrict__ dy, int B, int Hs, int Ws, int C,
                                                     float* __restrict__ out) {
    const long long total = (long long)B * Hs * Ws * C;
    const int W = 2 * Ws;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long p = i / C;
        const int xs = (int)(p % Ws);
        long long q = p / Ws;
        const int ys = (int)(q % Hs);
        const int b = (int)(q / Hs);
        const long long base = (((long long)b * 2 * Hs + 2 * ys) * W + 2 * xs) * C + c;
        out[i] = (dy[base] + dy[base + C]) + (dy[base + (long long)W * C] + dy[base + (long long)W * C + C]);
    }
}

// channel slice copy: out[m][0..Cs) = in[m][c0 .. c0+Cs)  (in has Cin channels)
__global__ __launch_bounds__(256) void slice_channels_kernel(const float* __restrict__ in, long long M, int Cin, int c0, int Cs,
                                                             float* __restrict__ out) {
    const long long total = M * Cs;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = in[(i / Cs) * Cin + c0 + (i % Cs)];
}

// out[m][0..Cin) = in[m][:], out[m][Cin..Cout) = 0
__global__ __launch_bounds__(256) void pad_channels_kernel(const float* __restrict__ in, long long M, int Cin, int Cout,
                                                           float* __restrict__ out) {
    const long long total = M * Cout;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cout);
        out[i] = c < Cin ? in[(i / Cout) * Cin + c] : 0.f;
    }
}

// forward packing with zero padding: dst[ci/32][tap][Npad][32] (every entry written)
__global__ void pack_fwd_padded_kernel(const float* __restrict__ w, int N, int C, int taps, int Cpad, int Npad,
                                       float* __restrict__ dst) {
    const long long total = (long long)Npad * Cpad * taps;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        long long t = i / taps;
        const int ci = (int)(t % Cpad), co = (int)(t / Cpad);
        const float v = (co < N && ci < C) ? w[((long long)co * C + ci) * taps + tap] : 0.f;
        dst[(((long long)(ci >> 5) * taps + tap) * Npad + co) * 32 + (ci & 31)] = v;
    }
}

// ------------------------------------------------------------------ weight gradient on the matrix cores
// dW[tap][ci][co] = sum_m X[pix(m) + tap][ci] * dY[m][co]:  per tap a GEMM [ci x M] * [M x co] with the
// reduction over pixels.  v_mfma_f32_32x32x2_f32 with k = 2 consecutive pixels: lanes 0-31 supply
// pixel p, lanes 32-63 pixel p+1, each lane one channel -> both operands are contiguous 128-B LDS rows.
struct WgradArgs {
    const float* src0; const float* src1;
    int C0, C1, ups, H, W, Hs, Ws, taps;
    const float* dy; int N;
    long long M;
    unsigned bytes0, bytes1;
    int ci_tiles, co_tiles;
    int chunks_total, chunks_per_split;    // 32-pixel chunks
    float* part;                           // [split][tap][Ctot][N]
};

template <int TI, int TJ>   // wave tile TI*32 (ci) x TJ*32 (co); workgroup = 2x2 waves
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradArgs a) {
    constexpr int CI_T = 2 * TI * 32, CO_T = 2 * TJ * 32, PK = 32;
    __shared__ __attribute__((aligned(16))) float xs[2][PK][CI_T];
    __shared__ __attribute__((aligned(16))) float ys[2][PK][CO_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int ci0 = (blockIdx.x / a.co_tiles) * CI_T, co0 = (blockIdx.x % a.co_tiles) * CO_T;
    const int tap = blockIdx.y;
    int dyy = 0, dxx = 0;
    if (a.taps == 9) { dyy = tap / 3 - 1; dxx = tap % 3 - 1; }
    const int Ctot = a.C0 + a.C1;
    const bool first = ci0 < a.C0;                       // a ci tile never straddles the concat boundary
    const int Cs = first ? a.C0 : a.C1;
    const int cbase = first ? ci0 : ci0 - a.C0;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(first ? a.src0 : a.src1), 0, first ? a.bytes0 : a.bytes1, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const int c_begin = blockIdx.z * a.chunks_per_split;
    const int c_end = min(c_begin + a.chunks_per_split, a.chunks_total);
    const int HW = a.H * a.W;
    // staging: X tile = PK rows x CI_T/4 float4, dY tile = PK rows x CO_T/4 float4
    constexpr int XV = PK * CI_T / 4 / 256, YV = PK * CO_T / 4 / 256;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    f32x4 gx[XV], gy[YV];
    auto load = [&](int chunk) {
        const long long m0 = (long long)chunk * PK;
#pragma unroll
        for (int k = 0; k < XV; ++k) {
            const int e = tid + 256 * k, row = e / (CI_T / 4), col4 = e % (CI_T / 4);
            const long long m = m0 + row;
            unsigned off = OOB;
            if (m < a.M) {
                const int b = (int)(m / HW), rem = (int)(m - (long long)b * HW);
                const int y = rem / a.W + dyy, x = rem % a.W + dxx;
                if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
                    off = (unsigned)(((b * a.Hs + (y >> a.ups)) * a.Ws + (x >> a.ups)) * Cs + cbase + col4 * 4) * 4u;
            }
            gx[k] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
#pragma unroll
        for (int k = 0; k < YV; ++k) {
            const int e = tid + 256 * k, row = e / (CO_T / 4), col4 = e % (CO_T / 4);
            const long long m = m0 + row;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < a.M) v = *reinterpret_cast<const f32x4*>(a.dy + m * a.N + co0 + col4 * 4);
            gy[k] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < XV; ++k) {
            const int e = tid + 256 * k;
            *reinterpret_cast<f32x4*>(&xs[buf][e / (CI_T / 4)][(e % (CI_T / 4)) * 4]) = gx[k];
        }
#pragma unroll
        for (int k = 0; k < YV; ++k) {
            const int e = tid + 256 * k;
            *reinterpret_cast<f32x4*>(&ys[buf][e / (CO_T / 4)][(e % (CO_T / 4)) * 4]) = gy[k];
        }
    };
    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (c_begin < c_end) { load(c_begin); store(0); }
    __syncthreads();
    int cur = 0;
    const int kh = lane >> 5, ln = lane & 31;
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = c + 1 < c_end;
        if (more) load(c + 1);
#pragma unroll
        for (int kk = 0; kk < PK / 2; ++kk) {
            float af[TI], bf[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) af[i] = xs[cur][2 * kk + kh][(wi * TI + i) * 32 + ln];
#pragma unroll
            for (int j = 0; j < TJ; ++j) bf[j] = ys[cur][2 * kk + kh][(wj * TJ + j) * 32 + ln];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (more) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    float* out = a.part + (((long long)blockIdx.z * a.taps + tap) * Ctot) * a.N;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + (wi * TI + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int co = co0 + (wj * TJ + j) * 32 + ln;
                out[(long long)ci * a.N + co] = acc[i][j][r];
            }
}

// ------------------------------------------------------------------ 3x3 weight gradient from an LDS-resident halo tile
// wgrad_kernel above runs one filter tap per workgroup: every tap re-reads X and dY and redoes the gather index
// arithmetic (two integer divisions per row per chunk).  Here a workgroup owns a 64 (ci) x 64 (co) block of dW for
// ALL nine taps (one 32x32 block per wave and tap: 9 accumulator tiles) and walks 2 x 32 pixel tiles of the images:
// per tile the 4 x 34 pixel halo of X (64 channels) and the 64 pixels of dY (64 channels) are DMA'd into LDS
// (buffer_load ... lds; out-of-image = out-of-range offset = zeros) and each pixel pair feeds nine MFMAs from one
// dY operand and nine shifted X operands.  Two workgroups share a CU; one computes while the other's tile loads.
struct WgradHaloArgs {
    const float* src0; const float* src1;
    int C0, C1, ups, H, W, Hs, Ws;
    const float* dy; int N;
    unsigned bytes0, bytes1, bytesy;
    int co_tiles;          // N / 64
    int n_tiles, splits;   // pixel tiles in total, workgroups sharing them (blockIdx.y)
    float* part;           // [split][tap][Ctot][N]
};
typedef __attribute__((address_space(3))) void* wg_lds_ptr_t;

__global__ __launch_bounds__(256, 2) void wgrad_halo_kernel(WgradHaloArgs a) {
    constexpr int HW_ = 34, XBYTES = 144 * 256;     // 4 x 34 halo pixels x 64 floats (36 DMA slots of 4 rows)
    extern __shared__ __attribute__((aligned(16))) char wlds[];
    char* const xs = wlds;
    char* const ys = wlds + XBYTES;                               // 64 pixels x 64 floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, kh = lane >> 5, ln = lane & 31;
    const int ci0 = (blockIdx.x / a.co_tiles) * 64, co0 = (blockIdx.x % a.co_tiles) * 64;
    const int Ctot = a.C0 + a.C1;
    const bool first = ci0 < a.C0;
    const int Cs = first ? a.C0 : a.C1;
    const int cbase = first ? ci0 : ci0 - a.C0;
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(first ? a.src0 : a.src1), 0, first ? a.bytes0 : a.bytes1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, a.bytesy, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const int tiles_x = a.W >> 5, tiles_y = a.H >> 1;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // DMA lane roles: a 1024-B instruction fills 4 rows of 256 B; lane -> (row lane/16, 16-B slot lane%16)
    const int drow = lane >> 4, dslot = lane & 15;
    for (int tile = blockIdx.y; tile < a.n_tiles; tile += a.splits) {
        int t = tile;
        const int tx = t % tiles_x; t /= tiles_x;
        const int ty = t % tiles_y;
        const int b = t / tiles_y;
        const int y0 = ty * 2, x0 = tx * 32;
        __syncthreads();                       // every wave is done with the previous tile
#pragma unroll
        for (int i = 0; i < 9; ++i) {          // X halo: slots q = 4 i + wave < 34 (136 rows)
            const int q = 4 * i + wave;
            if (q < 34) {
                const int hr = 4 * q + drow;
                const int hy = hr / HW_, hx = hr - hy * HW_;
                const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
                const bool ok = (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
                const unsigned off = ok ? (unsigned)(((b * a.Hs + (yy >> a.ups)) * a.Ws + (xx >> a.ups)) * Cs + cbase + dslot * 4) * 4u
                                        : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (wg_lds_ptr_t)(xs + q * 1024), 16, off, 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {          // dY: 64 pixels = 16 slots
            const int q = 4 * i + wave;
            const int p = 4 * q + drow;        // pixel of the tile: row p / 32, column p % 32
            const long long m = ((long long)b * a.H + y0 + (p >> 5)) * a.W + x0 + (p & 31);
            const unsigned off = (unsigned)((m * a.N + co0 + dslot * 4) * 4);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsy, (wg_lds_ptr_t)(ys + q * 1024), 16, off, 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const float* xw = reinterpret_cast<const float*>(xs) + wi * 32 + ln;
        const float* yw = reinterpret_cast<const float*>(ys) + wj * 32 + ln;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll 4
            for (int pp = 0; pp < 16; ++pp) {
                const int px = 2 * pp + kh;
                const float bv = yw[(r * 32 + px) * 64];
                const float* xr = xw + ((r * HW_) + px) * 64;          // halo pixel (r + dy', px + dx') for tap (0,0)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float av = xr[((tap / 3) * HW_ + (tap % 3)) * 64];
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tap], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        float* out = a.part + (((long long)blockIdx.y * 9 + tap) * Ctot) * a.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            out[(long long)ci * a.N + co0 + wj * 32 + ln] = acc[tap][r];
        }
    }
}

static bool wgrad_halo_ok(int H, int W, int ksize) { return ksize == 3 && H >= 2 && W >= 32 && !(H & 1) && !(W & 31); }
static void wgrad_halo_plan(int B, int H, int W, int Ctot, int N, int* n_tiles, int* splits) {
    *n_tiles = B * (H / 2) * (W / 32);
    const long long pairs = (long long)(Ctot / 64) * (N / 64);
    // one round of two workgroups per CU; more pixel splits only add partial slices for wgrad_reduce to read back
    constexpr int target = 512;
    long long s = nbp_cdiv(target, pairs);
    if (s > *n_tiles) s = *n_tiles;
    if (s > 1024) s = 1024;
    if (s < 1) s = 1;
    *splits = (int)s;
}

// dW OIHW [N][Creal][taps] = sum_s part[s][tap][ci][co]   (ci < Creal: padded input channels are dropped)
// One thread per (tap, ci, co) with co fastest: the reads of the `splits` slices are coalesced (the OIHW order made consecutive
// threads read Ctot * N floats apart: 104 us per call for 75 MB of partials); four slices in flight, added in slice order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int splits, int taps, int Ctot, int N,
                                                           int Creal, int Nreal, float* __restrict__ dw) {
    const long long total = (long long)Nreal * Creal * taps;
    const long long slice = (long long)taps * Ctot * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % Nreal);
        long long t = i / Nreal;
        const int ci = (int)(t % Creal), tap = (int)(t / Creal);
        const float* p = part + ((long long)tap * Ctot + ci) * N + co;
        float s = 0.f;
        int k = 0;
        for (; k + 4 <= splits; k += 4) {
            const float v0 = p[(long long)k * slice], v1 = p[(long long)(k + 1) * slice], v2 = p[(long long)(k + 2) * slice],
                        v3 = p[(long long)(k + 3) * slice];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < splits; ++k) s += p[(long long)k * slice];
        dw[((long long)co * Creal + ci) * taps + tap] = s;
    }
}

// First stage of a long slice reduction: out[g][i] = sum over the `group` consecutive slices of group g (slice order), 16 B per lane,
// four slices in flight.  With one 64 x 64 channel block a 256 x 256 layer leaves 512 slices of 147 KB, and one thread per output
// element walking all of them was a launch of 144 workgroups x 128 dependent round trips (50 us for 75 MB); 16 groups of 32 run on
// 16 x as many workgroups and the final pass reads 16 slices (round 5).
constexpr int WGRAD_REDUCE_GROUPS = 16;
__global__ __launch_bounds__(256) void slice_group_sum_kernel(const float* __restrict__ part, int splits, long long slice4, int group,
                                                              float* __restrict__ out) {
    const int g = blockIdx.y;
    const int k0 = g * group, k1 = min(k0 + group, splits);
    const f32x4* p = reinterpret_cast<const f32x4*>(part);
    f32x4* o = reinterpret_cast<f32x4*>(out) + (long long)g * slice4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slice4; i += (long long)gridDim.x * blockDim.x) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const f32x4 v0 = p[(long long)k * slice4 + i], v1 = p[(long long)(k + 1) * slice4 + i], v2 = p[(long long)(k + 2) * slice4 + i],
                        v3 = p[(long long)(k + 3) * slice4 + i];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < k1; ++k) s += p[(long long)k * slice4 + i];
        o[i] = s;
    }
}
// part [splits][taps][Ctot][N] -> dw OIHW; long reductions in two stages through `tmp` (WGRAD_REDUCE_GROUPS slices)
static int wgrad_reduce_launch(const float* part, int splits, int taps, int Ctot, int N, int c_real, int n_real, float* dw, float* tmp,
                               hipStream_t st) {
    const long long slice = (long long)taps * Ctot * N, total = (long long)n_real * c_real * taps;
    if (tmp && splits >= 4 * WGRAD_REDUCE_GROUPS && slice % 4 == 0) {
        const int group = (int)nbp_cdiv(splits, WGRAD_REDUCE_GROUPS), ng = (int)nbp_cdiv(splits, group);
        dim3 grid((unsigned)min(nbp_cdiv(slice / 4, 256), 1024ll), (unsigned)ng);
        slice_group_sum_kernel<<<grid, 256, 0, st>>>(part, splits, slice / 4, group, tmp);
        int rc = nbp_launch_status();
        if (rc) return rc;
        part = tmp; splits = ng;
    }
    wgrad_reduce_kernel<<<nbp_ew_grid(total, 256), 256, 0, st>>>(part, splits, taps, Ctot, N, c_real, n_real, dw);
    return nbp_launch_status();
}

// ------------------------------------------------------------------ weight gradient of Conv1.conv.0 (5 -> 64 channels, NCHW input)
// dW[co][c][tap] = sum over pixels of dY[p][co] x[c][p + tap]: a [64 x M] x [M x 45] product.  The step used to pad the network input
// from 5 to 64 channels and run the 64 -> 64 kernels on it (a 537-MB padded copy, a convolution and a weight gradient at 13 x the
// work); here a workgroup walks 8 x 32-pixel tiles like conv_first_mfma_kernel: the five 10 x 34 input planes and the tile's 256
// pixels of dY (64 KB, by DMA) sit in LDS, wave (wi, wj) owns the 32 (co) x 32 (k = c 9 + tap, 45 padded to 64) block and feeds
// v_mfma_f32_32x32x2_f32 with pixel pairs: A = dY^T (contiguous channels), B = the patch column of each lane (its own halo offset).
// Partial sums [workgroup][k][co]; the slice reduction writes OIHW.
constexpr int FW_PLANE = 10 * 34;
__global__ __launch_bounds__(256, 2) void wgrad_first_kernel(const float* __restrict__ x, int B, int H, int W, const float* __restrict__ dy,
                                                             unsigned dy_bytes, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char fl[];
    float* const hal = reinterpret_cast<float*>(fl);                       // [5][10][34] (+ pad)
    char* const ys = fl + 7168;                                            // [256 pixels][64 channels] fp32
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, kh = lane >> 5, ln = lane & 31;
    const int tiles_x = W >> 5, tiles_y = H >> 3, n_tiles = B * tiles_y * tiles_x;
    const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, dy_bytes, 0x00020000);
    const int k = wj * 32 + ln;                                            // this lane's column of the patch matrix
    const int koff = k < 45 ? (k / 9) * FW_PLANE + ((k % 9) / 3) * 34 + (k % 9) % 3 : -1;
    const int drow = lane >> 4, dslot = lane & 15;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        int tile = tile_id;
        const int tx = tile % tiles_x; tile /= tiles_x;
        const int ty = tile % tiles_y;
        const int b = tile / tiles_y;
        const int y0 = ty * 8, x0 = tx * 32;
        __syncthreads();                                                   // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < 16; ++i) {                                     // dY: 256 pixels x 256 B = 64 slots of 1 KB (4 pixels each)
            const int q = 4 * i + wave;
            const int p = 4 * q + drow;                                    // pixel of the tile: row p / 32, column p % 32
            const long long m = ((long long)b * H + y0 + (p >> 5)) * W + x0 + (p & 31);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsy, (wg_lds_ptr_t)(ys + q * 1024), 16, (unsigned)((m * 64 + dslot * 4) * 4), 0, 0, 0);
        }
        for (int i = tid; i < 5 * FW_PLANE; i += 256) {
            const int ci = i / FW_PLANE, r = i - ci * FW_PLANE;
            const int hy = r / 34, hx = r - hy * 34;
            const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
            hal[i] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? x[((long long)(b * 5 + ci) * H + yy) * W + xx] : 0.f;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const float* yw = reinterpret_cast<const float*>(ys) + wi * 32 + ln;
#pragma unroll 8
        for (int pp = 0; pp < 128; ++pp) {
            const int p = 2 * pp + kh;                                     // this half wave's pixel of the pair
            const float av = yw[p * 64];
            const float bv = koff >= 0 ? hal[koff + (p >> 5) * 34 + (p & 31)] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }
    // D[co][k]: row = co (the A side), column = k
    float* out = part + (long long)blockIdx.x * 64 * 64;                   // [k][co]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        out[(wj * 32 + ln) * 64 + co] = acc[r];
    }
}

// flipped + transposed packing for the data gradient: dst[(co)/32][tap][ci][co%32] = w[co][ci][taps-1-tap]
__global__ void pack_dgrad_kernel(const float* __restrict__ w, int N, int C, int taps, int Cpad, int Npad,
                                  float* __restrict__ dst) {
    const long long total = (long long)Npad * Cpad * taps;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        long long t = i / taps;
        const int ci = (int)(t % Cpad), co = (int)(t / Cpad);
        const float v = (co < N && ci < C) ? w[((long long)co * C + ci) * taps + (taps - 1 - tap)] : 0.f;
        dst[(((long long)(co >> 5) * taps + tap) * Cpad + ci) * 32 + (co & 31)] = v;
    }
}

// ------------------------------------------------------------------ loss pieces (nbp_model.py:162-173, nbp_utils.py:373-381)
// gather pred[k] = out1[b, c, x, y];  coords [K,4] int64 (b, c, x, y)
__global__ void gather_values_kernel(const float* __restrict__ out1, const long long* __restrict__ coords, int K, int Cc, int Hh,
                                     int Ww, float* __restrict__ pred) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const long long* q = coords + 4 * (long long)k;
    // (channel, row, col) are range-checked here, the batch index by the caller (the kernel does not know B); replay records
    // may come from a reference-format store written elsewhere
    const bool ok = q[0] >= 0 && q[1] >= 0 && q[1] < Cc && q[2] >= 0 && q[2] < Hh && q[3] >= 0 && q[3] < Ww;
    pred[k] = ok ? out1[((q[0] * Cc + q[1]) * Hh + q[2]) * Ww + q[3]] : 0.f;
}
// scatter-add grad into d_out1 (zeroed by the caller); duplicates accumulate (index_put accumulate=True semantics)
__global__ void scatter_values_kernel(const float* __restrict__ dpred, const long long* __restrict__ coords, int K, int Cc, int Hh,
                                      int Ww, float* __restrict__ dout1) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const long long* q = coords + 4 * (long long)k;
    if (!(q[0] >= 0 && q[1] >= 0 && q[1] < Cc && q[2] >= 0 && q[2] < Hh && q[3] >= 0 && q[3] < Ww)) return;
    atomicAdd(&dout1[((q[0] * Cc + q[1]) * Hh + q[2]) * Ww + q[3]], dpred[k]);
}
// partial sums of (p-t)^2 (mode 0) or BCE(p,t) with log clamped at -100 (mode 1, torch semantics)
__global__ __launch_bounds__(256) void loss_partial_kernel(int mode, const float* __restrict__ p, const float* __restrict__ t,
                                                           long long n, double* __restrict__ part) {
    __shared__ double sh[256];
    double s = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (mode == 0) { const float d = p[i] - t[i]; s += (double)(d * d); }
        else {
            const float lp = fmaxf(logf(p[i]), -100.f), l1 = fmaxf(logf(1.f - p[i]), -100.f);
            s += (double)(-(t[i] * lp + (1.f - t[i]) * l1));
        }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// d/dp: mode 0: coef * 2 (p - t) / n ;  mode 1: coef * (p - t) / (max(p (1-p), 1e-12)) / n
__global__ __launch_bounds__(256) void loss_grad_kernel(int mode, const float* __restrict__ p, const float* __restrict__ t,
                                                        long long n, float coef, float* __restrict__ dp) {
    const float inv = coef / (float)n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (mode == 0) dp[i] = 2.f * (p[i] - t[i]) * inv;
        else dp[i] = (p[i] - t[i]) / fmaxf(p[i] * (1.f - p[i]), 1e-12f) * inv;
    }
}

__global__ void sum_doubles_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < n; ++i) s += part[i];
        *out = s;
    }
}

inline int blocks_for_rows(long long M, long long* rows_per_block) {
    // >= 32 rows per block (the deep levels have few rows and many columns: M = 8192 x C = 1024 at batch 32 was 32 workgroups)
    long long nblk = M / 32;
    if (nblk < 1) nblk = 1;
    if (nblk > 1024) nblk = 1024;       // 4 workgroups per CU: the reductions are HBM streams
    *rows_per_block = nbp_cdiv(M, nblk);
    return (int)nbp_cdiv(M, *rows_per_block);
}

}  // namespace

// ================================================================== C ABI
extern "C" size_t nbp_colreduce_workspace_bytes(long long M, int C) {
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    return (size_t)nblk * 2 * C * sizeof(double) + (size_t)2 * C * sizeof(double) + 512;
}

// amax_out (or null): 64 zeroed words that receive max |y| (float bits; only for C % 4 == 0, else left untouched)
// stat_out (or null): [4 C] doubles that receive the UNROUNDED mean | invstd the normalisation used and, with relu, the two float
// bounds lo | hi of the channel's ReLU mask (y > 0 <=> lo <= x <= hi, MaskStat) -- handed to
// nbp_bn_train_backward_stat_f32, which rebuilds the ReLU mask from x with them instead of reading y
static int bn_forward_impl(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, int relu, float* mean,
                           float* invstd, float* y, void* amax_out_v, double* stat_out, void* ws, size_t ws_bytes, void* stream,
                           const double* ext_part = nullptr, int ext_rows = 0, const float* zero_row = nullptr);
extern "C" int nbp_bn_train_forward_amax_f32(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                                             float momentum, float* running_mean, float* running_var, int relu, float* mean,
                                             float* invstd, float* y, void* amax_out_v, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    return bn_forward_impl(x, M, C, gamma, beta, eps, momentum, running_mean, running_var, relu, mean, invstd, y, amax_out_v, nullptr, ws,
                           ws_bytes, stream);
}
// (the statistics buffer grew from [2 C] to [4 C] doubles in round 5 under an unchanged name and signature -- a caller built
// against the older contract would have been overrun silently.  The entry points carry the buffer's size now and a new name, so such
// a caller fails to link instead; and the two bounds are ALWAYS written -- without relu as (-inf, +inf), "every element passes" -- so
// that a backward asking for the mask on statistics of a forward that had none reads defined values.)
extern "C" int nbp_bn_train_forward_stat4_f32(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                                              float momentum, float* running_mean, float* running_var, int relu, float* mean,
                                              float* invstd, float* y, void* amax_out_v, double* stat_out, int stat_doubles, void* ws,
                                              size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!stat_out || ((uintptr_t)stat_out & 31), NBP_E_ARG);
    NBP_RETURN_IF(stat_doubles < 4 * C, NBP_E_WS);
    return bn_forward_impl(x, M, C, gamma, beta, eps, momentum, running_mean, running_var, relu, mean, invstd, y, amax_out_v, stat_out, ws,
                           ws_bytes, stream);
}
static int bn_forward_impl(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, int relu, float* mean,
                           float* invstd, float* y, void* amax_out_v, double* stat_out, void* ws, size_t ws_bytes, void* stream,
                           const double* ext_part, int ext_rows, const float* zero_row) {
    unsigned* amax_out = (unsigned*)amax_out_v;
    NBP_RETURN_IF(!x || !gamma || !beta || !mean || !invstd || !y || M < 1 || C < 1, NBP_E_ARG);
    hipStream_t st = (hipStream_t)stream;
    int rc = 0, nblk = ext_rows;
    const double* part = ext_part;
    double* stat_d = stat_out;
    if (!ext_part) {
        NBP_RETURN_IF(!ws || ws_bytes < nbp_colreduce_workspace_bytes(M, C), NBP_E_WS);
        long long rpb;
        nblk = blocks_for_rows(M, &rpb);
        double* p = (double*)(((uintptr_t)ws + 255) / 256 * 256);
        if (C % 4 == 0) colreduce4_kernel<0><<<nblk, 256, 0, st>>>(x, nullptr, nullptr, nullptr, nullptr, nullptr, M, C / 4, 0, rpb, p);
        else colreduce_kernel<0><<<nblk, 256, 0, st>>>(x, nullptr, nullptr, nullptr, nullptr, nullptr, M, C, 0, rpb, p);
        if ((rc = nbp_launch_status())) return rc;
        part = p;
        if (!stat_d) stat_d = p + (((size_t)nblk * 2 * C + 31) / 32 * 32);        // [2][C] unrounded mean, invstd (32-B aligned)
    }
    // (external partials -- the producing convolution's epilogue -- are sums of x and x^2 themselves: the shift row is zeros)
    // (stat_out: the caller's [4 C] doubles -- the ReLU mask's two bounds per channel are found here too)
    bn_finalize_kernel<<<(unsigned)nbp_cdiv(C, FIN_CH), 256, 0, st>>>(ext_part ? zero_row : x, part, nblk, C, M, eps, momentum, mean, invstd,
                                                                      running_mean, running_var, stat_d, (stat_out && relu) ? gamma : nullptr,
                                                                      beta, stat_out ? 1 : 0);
    if ((rc = nbp_launch_status())) return rc;
    if (C % 4 == 0) bn_apply4_kernel<<<nbp_ew_grid(M * C / 4, 256), 256, 0, st>>>(x, M * C / 4, C / 4, stat_d, gamma, beta, relu, y, amax_out);
    else bn_apply_kernel<<<nbp_ew_grid(M * C, 256), 256, 0, st>>>(x, M * C, C, stat_d, gamma, beta, relu, y);
    return nbp_launch_status();
}

// ... with the statistics' partial sums already written by the convolution that produced x (nbp_conv3x3_split_bn_f32 /
// nbp_upconv3x3_split_bn_f32: rows x [2][C] doubles of sum x, sum x^2): finalize + apply only, x is read once.  zero_row = C zeros.
extern "C" int nbp_bn_train_forward_part4_f32(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                                              float momentum, float* running_mean, float* running_var, int relu, float* mean,
                                              float* invstd, float* y, void* amax_out_v, double* stat_out, int stat_doubles,
                                              const double* part, int rows, const float* zero_row, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!stat_out || ((uintptr_t)stat_out & 31) || !part || rows < 1 || !zero_row, NBP_E_ARG);
    NBP_RETURN_IF(stat_doubles < 4 * C, NBP_E_WS);
    return bn_forward_impl(x, M, C, gamma, beta, eps, momentum, running_mean, running_var, relu, mean, invstd, y, amax_out_v, stat_out,
                           nullptr, 0, stream, part, rows, zero_row);
}

extern "C" int nbp_bn_train_forward_f32(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                                        float momentum, float* running_mean, float* running_var, int relu, float* mean,
                                        float* invstd, float* y, void* ws, size_t ws_bytes, void* stream) {
    return nbp_bn_train_forward_amax_f32(x, M, C, gamma, beta, eps, momentum, running_mean, running_var, relu, mean, invstd, y, nullptr,
                                         ws, ws_bytes, stream);
}

extern "C" int nbp_bn_train_backward_f32(const float* dy, const float* x, const float* y_or_null, long long M, int C,
                                         const float* mean, const float* invstd, const float* gamma, int relu, float* dx,
                                         float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    return nbp_bn_train_backward_fused_f32(dy, x, y_or_null, M, C, mean, invstd, gamma, relu, dx, dgamma, dbeta, nullptr, nullptr, ws,
                                           ws_bytes, stream);
}

// dx_colsum (or null; C floats) receives sum_m dx[m][c], amax_out (or null; 64 zeroed words) max |dx| -- both only for
// C % 4 == 0 (the caller checks nbp_bn_backward_fuses(C)); folded into the pass that writes dx.
extern "C" int nbp_bn_backward_fuses(int C) { return C % 4 == 0; }
static int bn_backward_impl(const float* dy, const float* x, const float* y_or_null, MaskStat ms, long long M, int C,
                            const float* mean, const float* invstd, const float* gamma, int relu, float* dx,
                            float* dgamma, float* dbeta, float* dx_colsum, void* amax_out_v, void* ws, size_t ws_bytes, void* stream);
extern "C" int nbp_bn_train_backward_fused_f32(const float* dy, const float* x, const float* y_or_null, long long M, int C,
                                               const float* mean, const float* invstd, const float* gamma, int relu, float* dx,
                                               float* dgamma, float* dbeta, float* dx_colsum, void* amax_out_v, void* ws,
                                               size_t ws_bytes, void* stream) {
    NBP_ENTER();
    return bn_backward_impl(dy, x, y_or_null, MaskStat{nullptr, nullptr, nullptr}, M, C, mean, invstd, gamma, relu, dx, dgamma, dbeta,
                            dx_colsum, amax_out_v, ws, ws_bytes, stream);
}
// The same with the ReLU mask rebuilt from x (read anyway) through the forward's unrounded statistics (stat_d of
// nbp_bn_train_forward_stat4_f32) and beta, instead of reading y: C % 4 == 0 only.
extern "C" int nbp_bn_train_backward_stat_f32(const float* dy, const float* x, const double* stat_d, const float* beta, long long M, int C,
                                              const float* mean, const float* invstd, const float* gamma, int relu, float* dx,
                                              float* dgamma, float* dbeta, float* dx_colsum, void* amax_out_v, void* ws,
                                              size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!stat_d || !beta || ((uintptr_t)stat_d & 31), NBP_E_ARG);
    NBP_RETURN_IF(C % 4 != 0, NBP_E_SHAPE);
    return bn_backward_impl(dy, x, nullptr, MaskStat{stat_d, gamma, beta}, M, C, mean, invstd, gamma, relu, dx, dgamma, dbeta, dx_colsum,
                            amax_out_v, ws, ws_bytes, stream);
}
static int bn_backward_impl(const float* dy, const float* x, const float* y_or_null, MaskStat ms, long long M, int C,
                            const float* mean, const float* invstd, const float* gamma, int relu, float* dx,
                            float* dgamma, float* dbeta, float* dx_colsum, void* amax_out_v, void* ws, size_t ws_bytes, void* stream) {
    unsigned* amax_out = (unsigned*)amax_out_v;
    NBP_RETURN_IF(!dy || !x || !mean || !invstd || !gamma || !dx || !dgamma || !dbeta || !ws || M < 1 || C < 1, NBP_E_ARG);
    NBP_RETURN_IF(relu && !y_or_null && !ms.stat_d, NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_colreduce_workspace_bytes(M, C), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    if (C % 4 == 0) colreduce4_kernel<1><<<nblk, 256, 0, st>>>(dy, x, y_or_null, mean, invstd, nullptr, M, C / 4, relu, rpb, part, ms);
    else colreduce_kernel<1><<<nblk, 256, 0, st>>>(dy, x, y_or_null, mean, invstd, nullptr, M, C, relu, rpb, part);
    int rc = nbp_launch_status();
    if (rc) return rc;
    double* sums = part + (((size_t)nblk * 2 * C + 31) / 32 * 32);          // [2][C] unrounded dbeta, dgamma (32-B aligned)
    // (the float4 reduction leaves sum dz x: turned into sum dz xhat by the finalizer)
    colsum_finalize_kernel<<<(unsigned)nbp_cdiv(C, FIN_CH), 256, 0, st>>>(part, nblk, C, dbeta, dgamma, sums, C % 4 == 0 ? mean : nullptr,
                                                                          C % 4 == 0 ? invstd : nullptr);
    if ((rc = nbp_launch_status())) return rc;
    if (C % 4 == 0 && (dx_colsum || amax_out)) {
        // dx, its column sums and its max |.| in ONE pass (the partials reuse `part`: the finalizer above has consumed it)
        bn_backward_apply4_sum_kernel<<<nblk, 256, 0, st>>>(dy, x, y_or_null, M, C / 4, mean, invstd, gamma, sums, relu, rpb, dx, part,
                                                            amax_out, ms);
        if ((rc = nbp_launch_status())) return rc;
        if (dx_colsum) {
            colsum_finalize_kernel<<<(unsigned)nbp_cdiv(C, FIN_CH), 256, 0, st>>>(part, nblk, C, dx_colsum, nullptr);
            rc = nbp_launch_status();
        }
        return rc;
    }
    if (C % 4 == 0)
        bn_backward_apply4_kernel<<<nbp_ew_grid(M * C / 4, 256), 256, 0, st>>>(dy, x, y_or_null, M * C / 4, C / 4, M, mean, invstd,
                                                                              gamma, sums, relu, dx, ms);
    else
        bn_backward_apply_kernel<<<nbp_ew_grid(M * C, 256), 256, 0, st>>>(dy, x, y_or_null, M * C, C, M, mean, invstd, gamma,
                                                                         sums, relu, dx);
    return nbp_launch_status();
}

// ---- the attention gate's element-wise middle in training (kernels above).  F = F_int: a multiple of 4 with F / 4 a power of two
// <= 64 (32, 64, 128, 256 in the network).  stat_g / stat_x: [4 F] doubles each (unrounded mean | invstd | -inf | +inf, as
// nbp_bn_train_forward_stat4_f32 writes them without relu); mean_* / invstd_*: [F] floats for the backward.
extern "C" size_t nbp_gate_mid_workspace_bytes(long long M, int F) {
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    return (size_t)nblk * 4 * F * sizeof(double) + (size_t)4 * F * sizeof(double) + 1024;
}
static bool gate_mid_shape_ok(long long M, int F) {
    if (M < 1 || F < 4 || F % 4 != 0) return false;
    const int F4 = F / 4;
    return F4 >= 4 && F4 <= 64 && (F4 & (F4 - 1)) == 0 && M * F < (1ll << 40);
}
extern "C" int nbp_gate_mid_forward_f32(const float* g_pre, const float* x_pre, long long M, int F,
                                        const float* gamma_g, const float* beta_g, float* run_mean_g, float* run_var_g, float eps_g, float mom_g,
                                        const float* gamma_x, const float* beta_x, float* run_mean_x, float* run_var_x, float eps_x, float mom_x,
                                        float* mean_g, float* invstd_g, float* mean_x, float* invstd_x, double* stat_g, double* stat_x,
                                        const float* w_psi, const float* b_psi, float* q, float* p, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!g_pre || !x_pre || !gamma_g || !beta_g || !gamma_x || !beta_x || !mean_g || !invstd_g || !mean_x || !invstd_x || !stat_g ||
                  !stat_x || !w_psi || !b_psi || !q || !p || !ws, NBP_E_ARG);
    NBP_RETURN_IF(!gate_mid_shape_ok(M, F), NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)g_pre | (uintptr_t)x_pre | (uintptr_t)q | (uintptr_t)w_psi | (uintptr_t)gamma_g | (uintptr_t)beta_g |
                    (uintptr_t)gamma_x | (uintptr_t)beta_x) & 15) || (((uintptr_t)stat_g | (uintptr_t)stat_x) & 31), NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_gate_mid_workspace_bytes(M, F), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    int rc;
    for (int which = 0; which < 2; ++which) {          // the two BatchNorms' statistics (one read of each tensor)
        const float* src = which ? x_pre : g_pre;
        colreduce4_kernel<0><<<nblk, 256, 0, st>>>(src, nullptr, nullptr, nullptr, nullptr, nullptr, M, F / 4, 0, rpb, part);
        if ((rc = nbp_launch_status())) return rc;
        bn_finalize_kernel<<<(unsigned)nbp_cdiv(F, FIN_CH), 256, 0, st>>>(src, part, nblk, F, M, which ? eps_x : eps_g, which ? mom_x : mom_g,
                                                                          which ? mean_x : mean_g, which ? invstd_x : invstd_g,
                                                                          which ? run_mean_x : run_mean_g, which ? run_var_x : run_var_g,
                                                                          which ? stat_x : stat_g, nullptr, which ? beta_x : beta_g, 1);
        if ((rc = nbp_launch_status())) return rc;
    }
    const int F4 = F / 4, rows_pb = 256 / F4;
    long long blocks = (M + 2ll * rows_pb - 1) / (2ll * rows_pb);
    if (blocks > 4096) blocks = 4096;
    gate_mid_fwd4_kernel<<<(unsigned)blocks, 256, 0, st>>>(g_pre, x_pre, M, F4, GateBn{stat_g, stat_x, gamma_g, beta_g, gamma_x, beta_x}, w_psi,
                                                           b_psi, q, p);
    return nbp_launch_status();
}

// dp [M] = the gradient of p.  Outputs: d g_pre, d x_pre [M, F]; dgamma / dbeta of both BatchNorms; dw_psi [F]; csum_g / csum_x [F] =
// the column sums of d g_pre / d x_pre (the 1x1 convolutions' bias gradients); amax_g / amax_x (or null): 64 zeroed words each that
// receive max |d g_pre| / max |d x_pre|.
extern "C" int nbp_gate_mid_backward_f32(const float* dp, const float* w_psi, const float* q, const float* g_pre, const float* x_pre,
                                         long long M, int F, const float* mean_g, const float* invstd_g, const float* gamma_g,
                                         const float* mean_x, const float* invstd_x, const float* gamma_x, float* dg_pre, float* dx_pre,
                                         float* dgamma_g, float* dbeta_g, float* dgamma_x, float* dbeta_x, float* dw_psi, float* csum_g,
                                         float* csum_x, void* amax_g, void* amax_x, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!dp || !w_psi || !q || !g_pre || !x_pre || !mean_g || !invstd_g || !gamma_g || !mean_x || !invstd_x || !gamma_x || !dg_pre ||
                  !dx_pre || !dgamma_g || !dbeta_g || !dgamma_x || !dbeta_x || !dw_psi || !csum_g || !csum_x || !ws, NBP_E_ARG);
    NBP_RETURN_IF(!gate_mid_shape_ok(M, F), NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)q | (uintptr_t)g_pre | (uintptr_t)x_pre | (uintptr_t)dg_pre | (uintptr_t)dx_pre | (uintptr_t)w_psi |
                    (uintptr_t)mean_g | (uintptr_t)invstd_g | (uintptr_t)gamma_g | (uintptr_t)mean_x | (uintptr_t)invstd_x |
                    (uintptr_t)gamma_x) & 15), NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_gate_mid_workspace_bytes(M, F), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    double* sums_g = part + (((size_t)nblk * 4 * F + 31) / 32 * 32);
    double* sums_x = sums_g + 2 * (size_t)F;
    gate_mid_bwd_reduce4_kernel<<<nblk, 256, 0, st>>>(dp, w_psi, q, g_pre, x_pre, M, F / 4, part);
    int rc = nbp_launch_status();
    if (rc) return rc;
    gate_mid_bwd_finalize_kernel<<<(unsigned)nbp_cdiv(F, FIN_CH), 256, 0, st>>>(part, nblk, F, mean_g, invstd_g, mean_x, invstd_x, dbeta_g,
                                                                                dgamma_g, dbeta_x, dgamma_x, dw_psi, sums_g, sums_x);
    if ((rc = nbp_launch_status())) return rc;
    gate_mid_bwd_apply4_kernel<<<nblk, 256, 0, st>>>(dp, w_psi, q, g_pre, x_pre, M, F / 4, mean_g, invstd_g, gamma_g, sums_g, mean_x, invstd_x,
                                                     gamma_x, sums_x, dg_pre, dx_pre, part, (unsigned*)amax_g, (unsigned*)amax_x);
    if ((rc = nbp_launch_status())) return rc;
    colsum_finalize_kernel<<<(unsigned)nbp_cdiv(F, FIN_CH), 256, 0, st>>>(part, nblk, F, csum_g, csum_x);
    return nbp_launch_status();
}

// out[c] = sum_m rows[m] * x[m][c]  (rows may be null): bias gradients, psi weight gradient
extern "C" int nbp_colsum_f32(const float* x, const float* rows_or_null, long long M, int C, float* out, void* ws,
                              size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !out || !ws || M < 1 || C < 1, NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_colreduce_workspace_bytes(M, C), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    long long rpb;
    const int nblk = blocks_for_rows(M, &rpb);
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    if (C % 4 == 0) colreduce4_kernel<2><<<nblk, 256, 0, st>>>(x, nullptr, nullptr, nullptr, nullptr, rows_or_null, M, C / 4, 0, rpb, part);
    else colreduce_kernel<2><<<nblk, 256, 0, st>>>(x, nullptr, nullptr, nullptr, nullptr, rows_or_null, M, C, 0, rpb, part);
    int rc = nbp_launch_status();
    if (rc) return rc;
    colsum_finalize_kernel<<<(unsigned)nbp_cdiv(C, FIN_CH), 256, 0, st>>>(part, nblk, C, out, nullptr);
    return nbp_launch_status();
}

extern "C" int nbp_elementwise_f32(int op, const float* a, const float* b, long long n, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!a || !out || n < 1 || op < 0 || op > 5, NBP_E_ARG);
    NBP_RETURN_IF(op != 2 && !b, NBP_E_ARG);
    const bool al16 = (((uintptr_t)a | (uintptr_t)out | (uintptr_t)(op == 2 || op == 5 ? a : b)) & 15) == 0;
    if (n % 4 == 0 && al16) ew4_kernel<<<nbp_ew_grid(n / 4, 256), 256, 0, (hipStream_t)stream>>>(op, a, b, n / 4, out);
    else ew_kernel<<<nbp_ew_grid(n, 256), 256, 0, (hipStream_t)stream>>>(op, a, b, n, out);
    return nbp_launch_status();
}

extern "C" int nbp_sum_n_f32(int n, const float* const* srcs_host, const long long* ld_host, long long M, int C, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(n < 1 || n > SUM_N_MAX || !srcs_host || !ld_host || !out || M < 1 || C < 4 || C % 4 != 0 || ((uintptr_t)out & 15), NBP_E_ARG);
    SumNArgs a = {};
    a.n = n;
    for (int k = 0; k < n; ++k) {
        NBP_RETURN_IF(!srcs_host[k] || ((uintptr_t)srcs_host[k] & 15) || ld_host[k] < C || ld_host[k] % 4 != 0, NBP_E_ARG);
        a.src[k] = srcs_host[k]; a.ld4[k] = ld_host[k] / 4;
    }
    {
        const int C4 = C / 4, rpb = 256 / (C4 < 256 ? C4 : 256);
        long long blocks = (M + 2ll * rpb - 1) / (2ll * rpb);
        if (blocks > 8192) blocks = 8192;
        sum_n4_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a, M, C4, out);
    }
    return nbp_launch_status();
}

extern "C" int nbp_rowscale_f32(const float* x, const float* s, long long M, int C, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !s || !out || M < 1 || C < 1, NBP_E_ARG);
    if (C % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0)
        rowscale4_kernel<<<nbp_ew_grid(M * C / 4, 256), 256, 0, (hipStream_t)stream>>>(x, s, M * C / 4, C / 4, out);
    else
        rowscale_kernel<<<nbp_ew_grid(M * C, 256), 256, 0, (hipStream_t)stream>>>(x, s, M * C, C, out);
    return nbp_launch_status();
}
// ... that also leaves max |out| in the 64 zeroed words of amax_out (C % 4 == 0, 16-byte aligned tensors)
extern "C" int nbp_rowscale_amax_f32(const float* x, const float* s, long long M, int C, float* out, void* amax_out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !s || !out || !amax_out || M < 1 || C < 4, NBP_E_ARG);
    NBP_RETURN_IF((C & 3) || (((uintptr_t)x | (uintptr_t)out) & 15), NBP_E_SHAPE);
    rowscale4_kernel<<<nbp_ew_grid(M * C / 4, 256), 256, 0, (hipStream_t)stream>>>(x, s, M * C / 4, C / 4, out, (unsigned*)amax_out);
    return nbp_launch_status();
}

extern "C" int nbp_rowscale_backward_f32(const float* dy, long long ldy, const float* x, const float* s, long long M, int C, float* dx,
                                         float* ds, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!dy || !x || !s || !dx || !ds || M < 1 || C < 4, NBP_E_ARG);
    NBP_RETURN_IF((C & 3) || (ldy & 3) || ldy < C || (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx) & 15), NBP_E_SHAPE);
    rowscale_bwd4_kernel<<<nbp_ew_grid(M * 16, 256), 256, 0, (hipStream_t)stream>>>(dy, ldy / 4, x, s, M, C / 4, dx, ds);
    return nbp_launch_status();
}

extern "C" int nbp_rowdot_f32(const float* a, const float* b, int b_is_vector, long long M, int C, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!a || !b || !out || M < 1 || C < 1, NBP_E_ARG);
    rowdot_kernel<<<nbp_ew_grid(M * 16, 256), 256, 0, (hipStream_t)stream>>>(a, b, b_is_vector, M, C, out);
    return nbp_launch_status();
}

extern "C" int nbp_outer_f32(const float* s, const float* w, long long M, int C, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!s || !w || !out || M < 1 || C < 1, NBP_E_ARG);
    outer_kernel<<<nbp_ew_grid(M * C, 256), 256, 0, (hipStream_t)stream>>>(s, w, M * C, C, out);
    return nbp_launch_status();
}

extern "C" int nbp_maxpool2_backward_f32(const float* x, const float* dy, int B, int H, int W, int C, float* dx, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !dy || !dx, NBP_E_ARG);
    NBP_RETURN_IF(B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1, NBP_E_SHAPE);
    if (C % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0)
        maxpool2_bwd4_kernel<<<nbp_ew_grid((long long)B * (H / 2) * (W / 2) * C / 4, 256), 256, 0, (hipStream_t)stream>>>(
            x, dy, B, H, W, C / 4, dx);
    else
        maxpool2_bwd_kernel<<<nbp_ew_grid((long long)B * (H / 2) * (W / 2) * C, 256), 256, 0, (hipStream_t)stream>>>(x, dy, B, H, W,
                                                                                                                 C, dx);
    return nbp_launch_status();
}

extern "C" int nbp_sum2x2_f32(const float* dy, int B, int Hs, int Ws, int C, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!dy || !out || B < 1 || Hs < 1 || Ws < 1 || C < 1, NBP_E_ARG);
    if (C % 4 == 0 && (((uintptr_t)dy | (uintptr_t)out) & 15) == 0)
        sum2x2_4_kernel<<<nbp_ew_grid((long long)B * Hs * Ws * C / 4, 256), 256, 0, (hipStream_t)stream>>>(dy, B, Hs, Ws, C / 4, out);
    else
        sum2x2_kernel<<<nbp_ew_grid((long long)B * Hs * Ws * C, 256), 256, 0, (hipStream_t)stream>>>(dy, B, Hs, Ws, C, out);
    return nbp_launch_status();
}

extern "C" int nbp_slice_channels_f32(const float* in, long long M, int Cin, int c0, int Cs, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!in || !out || M < 1 || Cin < 1 || c0 < 0 || Cs < 1 || c0 + Cs > Cin, NBP_E_ARG);
    if (Cin % 4 == 0 && c0 % 4 == 0 && Cs % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0)
        slice_channels4_kernel<<<nbp_ew_grid(M * Cs / 4, 256), 256, 0, (hipStream_t)stream>>>(in, M, Cin / 4, c0 / 4, Cs / 4, out);
    else
        slice_channels_kernel<<<nbp_ew_grid(M * Cs, 256), 256, 0, (hipStream_t)stream>>>(in, M, Cin, c0, Cs, out);
    return nbp_launch_status();
}

extern "C" int nbp_pad_channels_f32(const float* in, long long M, int Cin, int Cout, float* out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!in || !out || M < 1 || Cin < 1 || Cout < Cin, NBP_E_ARG);
    pad_channels_kernel<<<nbp_ew_grid(M * Cout, 256), 256, 0, (hipStream_t)stream>>>(in, M, Cin, Cout, out);
    return nbp_launch_status();
}

extern "C" int nbp_pack_conv_weight_padded(const float* w_oihw, int N, int C, int ksize, int Cpad, int Npad, float* dst,
                                           void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!w_oihw || !dst || N < 1 || C < 1 || (ksize != 1 && ksize != 3), NBP_E_ARG);
    NBP_RETURN_IF(Cpad < C || Cpad % 32 || Npad < N || Npad % 32, NBP_E_SHAPE);
    const long long total = (long long)Npad * Cpad * ksize * ksize;
    pack_fwd_padded_kernel<<<nbp_ew_grid(total, 256), 256, 0, (hipStream_t)stream>>>(w_oihw, N, C, ksize * ksize, Cpad, Npad,
                                                                                    dst);
    return nbp_launch_status();
}

extern "C" int nbp_pack_conv_weight_dgrad(const float* w_oihw, int N, int C, int ksize, int Cpad, int Npad, float* dst,
                                          void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!w_oihw || !dst || N < 1 || C < 1 || (ksize != 1 && ksize != 3), NBP_E_ARG);
    NBP_RETURN_IF(Cpad < C || Cpad % 32 || Npad < N || Npad % 32, NBP_E_SHAPE);
    const long long total = (long long)Npad * Cpad * ksize * ksize;
    pack_dgrad_kernel<<<nbp_ew_grid(total, 256), 256, 0, (hipStream_t)stream>>>(w_oihw, N, C, ksize * ksize, Cpad, Npad, dst);
    return nbp_launch_status();
}

static void wgrad_plan(long long M, int Ctot, int N, int taps, int* ti, int* ci_tiles, int* co_tiles, int* splits,
                       int* chunks_total, int* cps) {
    *ti = (Ctot % 128 == 0 && N % 128 == 0) ? 2 : 1;       // 128x128 or 64x64 workgroup tile
    const int T = *ti * 64;
    *ci_tiles = Ctot / T; *co_tiles = N / T;
    *chunks_total = (int)nbp_cdiv(M, 32);
    const long long base = (long long)*ci_tiles * *co_tiles * taps;
    long long s = nbp_cdiv(1024, base);
    if (s > *chunks_total) s = *chunks_total;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    *cps = (int)nbp_cdiv(*chunks_total, s);
    *splits = (int)nbp_cdiv(*chunks_total, *cps);
}

extern "C" size_t nbp_conv_wgrad_workspace_bytes(int B, int H, int W, int C0, int C1, int N, int ksize) {
    int ti, cit, cot, sp, ct, cps;
    if (ksize == 1 && C1 == 0 && C0 % 64 == 0 && C0 <= 128 && N % 4 == 0 && N % 64) {      // the 1x1 split form alone takes such N
        const long long M1 = (long long)B * H * W, n_tiles = M1 / 64;
        long long s1 = nbp_cdiv(1024, (long long)(C0 / 64) * ((N + 63) / 64));
        if (s1 > n_tiles) s1 = n_tiles;
        return (size_t)(s1 + WGRAD_REDUCE_GROUPS) * C0 * N * sizeof(float) + 256 + 1024;
    }
    if ((C0 + C1) % 64 || N % 64 || C0 % 64) return 0;
    wgrad_plan((long long)B * H * W, C0 + C1, N, ksize * ksize, &ti, &cit, &cot, &sp, &ct, &cps);
    if (wgrad_halo_ok(H, W, ksize)) {
        int nt, hs;
        wgrad_halo_plan(B, H, W, C0 + C1, N, &nt, &hs);
        if (hs > sp) sp = hs;
    } else if (ksize == 3 && H >= 4 && W >= 16 && !(H & 3) && !(W & 15)) {      // the split form's 4 x 16 tiles
        int nt, hs;
        wgrad_halo_plan(B, H / 2, W * 2, C0 + C1, N, &nt, &hs);
        if (hs > sp) sp = hs;
    }
    if (ksize == 1 && C1 == 0 && C0 <= 128) {                      // the 1x1 split form: up to 1024 slices
        const long long M1 = (long long)B * H * W, n_tiles = M1 / 64;
        long long s1 = nbp_cdiv(1024, (long long)(C0 / 64) * (N / 64));
        if (s1 > n_tiles) s1 = n_tiles;
        if (s1 > sp) sp = (int)s1;
    }
    // (+ max-|.| scratch of the split form, + the first-stage sums of a long slice reduction)
    return (size_t)(sp + WGRAD_REDUCE_GROUPS) * ksize * ksize * (C0 + C1) * N * sizeof(float) + 256 + 1024;
}

// dW [n_real][c_real][k][k] (OIHW) of out = conv(cat(src0, src1) [upsampled]) given dY [B,H,W,N].
// C0, C1, N multiples of 64 (pad small layers); c_real / n_real select the un-padded part written.
extern "C" int nbp_conv_wgrad_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W, int ksize,
                                  const float* dy, int N, int c_real, int n_real, float* dw, void* ws, size_t ws_bytes,
                                  void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!src0 || !dy || !dw || !ws || B < 1 || H < 1 || W < 1, NBP_E_ARG);
    NBP_RETURN_IF(ksize != 1 && ksize != 3, NBP_E_ARG);
    NBP_RETURN_IF(C0 < 64 || C0 % 64 || C1 < 0 || C1 % 64 || N < 64 || N % 64, NBP_E_SHAPE);
    NBP_RETURN_IF((C1 > 0 && !src1) || c_real < 1 || c_real > C0 + C1 || n_real < 1 || n_real > N, NBP_E_ARG);
    NBP_RETURN_IF(ups && ((H | W) & 1), NBP_E_SHAPE);
    WgradArgs a;
    a.src0 = src0; a.src1 = src1; a.C0 = C0; a.C1 = C1; a.ups = ups ? 1 : 0; a.H = H; a.W = W;
    a.Hs = ups ? H / 2 : H; a.Ws = ups ? W / 2 : W; a.taps = ksize * ksize; a.dy = dy; a.N = N;
    a.M = (long long)B * H * W;
    const long long b0 = (long long)B * a.Hs * a.Ws * C0 * 4, b1 = (long long)B * a.Hs * a.Ws * C1 * 4;
    NBP_RETURN_IF(b0 >= (1ll << 31) || b1 >= (1ll << 31), NBP_E_SHAPE);
    a.bytes0 = (unsigned)b0; a.bytes1 = C1 ? (unsigned)b1 : (unsigned)b0;
    hipStream_t st = (hipStream_t)stream;
    if (wgrad_halo_ok(H, W, ksize) && (long long)B * H * W * N * 4 < (1ll << 31)) {
        WgradHaloArgs h;
        h.src0 = src0; h.src1 = src1; h.C0 = C0; h.C1 = C1; h.ups = a.ups; h.H = H; h.W = W; h.Hs = a.Hs; h.Ws = a.Ws;
        h.dy = dy; h.N = N; h.bytes0 = a.bytes0; h.bytes1 = a.bytes1; h.bytesy = (unsigned)((long long)B * H * W * N * 4);
        h.co_tiles = N / 64;
        wgrad_halo_plan(B, H, W, C0 + C1, N, &h.n_tiles, &h.splits);
        NBP_RETURN_IF(ws_bytes < (size_t)h.splits * 9 * (C0 + C1) * N * sizeof(float) + 256, NBP_E_WS);
        h.part = (float*)(((uintptr_t)ws + 255) / 256 * 256);
        constexpr int smem = 144 * 256 + 64 * 256;
        static bool attr_set = false;
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_halo_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, smem);
            if (e != hipSuccess) return (int)e;
            attr_set = true;
        }
        dim3 grid((unsigned)(((C0 + C1) / 64) * (N / 64)), (unsigned)h.splits);
        wgrad_halo_kernel<<<grid, 256, smem, st>>>(h);
        int rc = nbp_launch_status();
        if (rc) return rc;
        float* tmp = h.part + (size_t)h.splits * 9 * (C0 + C1) * N;
        const bool room = ws_bytes >= (size_t)(h.splits + WGRAD_REDUCE_GROUPS) * 9 * (C0 + C1) * N * sizeof(float) + 256;
        return wgrad_reduce_launch(h.part, h.splits, 9, C0 + C1, N, c_real, n_real, dw, room ? tmp : nullptr, st);
    }
    int ti, sp;
    wgrad_plan(a.M, C0 + C1, N, a.taps, &ti, &a.ci_tiles, &a.co_tiles, &sp, &a.chunks_total, &a.chunks_per_split);
    NBP_RETURN_IF(ti == 2 && C0 % 128, NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < (size_t)sp * a.taps * (C0 + C1) * N * sizeof(float) + 256, NBP_E_WS);
    a.part = (float*)(((uintptr_t)ws + 255) / 256 * 256);
    dim3 grid((unsigned)(a.ci_tiles * a.co_tiles), (unsigned)a.taps, (unsigned)sp);
    if (ti == 2) wgrad_kernel<2, 2><<<grid, 256, 0, st>>>(a);
    else wgrad_kernel<1, 1><<<grid, 256, 0, st>>>(a);
    int rc = nbp_launch_status();
    if (rc) return rc;
    {
        float* tmp = a.part + (size_t)sp * a.taps * (C0 + C1) * N;
        const bool room = ws_bytes >= (size_t)(sp + WGRAD_REDUCE_GROUPS) * a.taps * (C0 + C1) * N * sizeof(float) + 256;
        return wgrad_reduce_launch(a.part, sp, a.taps, C0 + C1, N, c_real, n_real, dw, room ? tmp : nullptr, st);
    }
}

// dW [64][5][3][3] of Conv1.conv.0 from the network input x [B,5,H,W] (NCHW, as the forward reads it) and dy [B,H,W,64]; H % 8 == 0,
// W % 32 == 0.  Workspace: nbp_conv_first_wgrad_workspace_bytes.
constexpr int FW_GRID = 512;
extern "C" size_t nbp_conv_first_wgrad_workspace_bytes(void) { return 256 + (size_t)(FW_GRID + WGRAD_REDUCE_GROUPS) * 64 * 64 * sizeof(float); }
extern "C" int nbp_conv_first_wgrad_f32(const float* x_nchw, int B, int H, int W, const float* dy, float* dw, void* ws, size_t ws_bytes,
                                        void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x_nchw || !dy || !dw || !ws || B < 1, NBP_E_ARG);
    NBP_RETURN_IF(H < 8 || W < 32 || (H & 7) || (W & 31), NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < nbp_conv_first_wgrad_workspace_bytes(), NBP_E_WS);
    const long long by = (long long)B * H * W * 64 * 4;
    NBP_RETURN_IF(by >= (1ll << 31), NBP_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)(((uintptr_t)ws + 255) / 256 * 256);
    const int n_tiles = B * (H / 8) * (W / 32), grid = n_tiles < FW_GRID ? n_tiles : FW_GRID;
    constexpr int smem = 7168 + 256 * 256;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_first_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    wgrad_first_kernel<<<grid, 256, smem, st>>>(x_nchw, B, H, W, dy, (unsigned)by, part);
    int rc = nbp_launch_status();
    if (rc) return rc;
    // slices [grid][k = 64][co = 64] -> dw[co][k < 45]
    return wgrad_reduce_launch(part, grid, 1, 64, 64, 45, 64, dw, part + (size_t)grid * 64 * 64, st);
}

// (nbp_split.hip)
int nbp_wgrad_1x1_split_launch(const float* x, int C, long long M, const float* dy, int N, int n_tiles, int splits, const unsigned* amax_x,
                               const unsigned* amax_y, float* part, hipStream_t st, int one);
int nbp_wgrad_split_launch(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W, const float* dy, int N,
                           int n_tiles, int splits, unsigned* amax3, const unsigned* amax0_in, const unsigned* amax1_in,
                           const unsigned* amaxy_in, float* part, hipStream_t st, int one);

// The same gradient with the products on the fp16 matrix pipe (two-piece operands, three exact MFMAs per product, fp32
// accumulation; nbp_split.hip: wgrad_split_kernel) for the 3x3 layers the halo-tile form takes; everything else falls through
// to nbp_conv_wgrad_f32.  Workspace: nbp_conv_wgrad_workspace_bytes (it includes the 768 B of max-|.| scratch).
static int conv_wgrad_split_impl(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                                 int ksize, const float* dy, int N, int c_real, int n_real, float* dw,
                                 const void* amax0_or_null, const void* amax1_or_null, const void* amaxy_or_null, void* ws,
                                 size_t ws_bytes, void* stream, int one) {
    const bool wide = wgrad_halo_ok(H, W, ksize), narrow = !wide && ksize == 3 && H >= 4 && W >= 16 && !(H & 3) && !(W & 15);
    const bool take = ksize == 3 && (wide || narrow) && (long long)B * H * W * N * 4 < (1ll << 31) && src0 && dy && dw &&
                      ws && B >= 1 && C0 >= 64 && C0 % 64 == 0 && C1 >= 0 && C1 % 64 == 0 && N >= 64 && N % 64 == 0 &&
                      (C1 == 0 || src1) && !(ups && ((H | W) & 1));
    // 1x1 layers on the large levels (few channels, many pixels: memory-bound) run the split scheme's own kernel; N need not be padded
    const long long M1 = (long long)B * H * W;
    if (ksize == 1 && C1 == 0 && !ups && src0 && dy && dw && ws && amax0_or_null && amaxy_or_null && C0 >= 64 && C0 % 64 == 0 && C0 <= 128 &&
        N >= 4 && N % 4 == 0 && c_real == C0 && n_real == N && M1 % 64 == 0 && M1 * C0 * 4 < (1ll << 31) && M1 * N * 4 < (1ll << 31)) {
        NBP_ENTER();
        const int n_tiles = (int)(M1 / 64);
        const long long pairs = (long long)(C0 / 64) * ((N + 63) / 64);
        long long sp = nbp_cdiv(1024, pairs);
        if (sp > n_tiles) sp = n_tiles;
        const size_t slice = (size_t)C0 * N * sizeof(float);
        if (ws_bytes >= (size_t)(sp + WGRAD_REDUCE_GROUPS) * slice + 256) {
            float* part = (float*)(((uintptr_t)ws + 255) / 256 * 256);
            hipStream_t st1 = (hipStream_t)stream;
            int rc = nbp_wgrad_1x1_split_launch(src0, C0, M1, dy, N, n_tiles, (int)sp, (const unsigned*)amax0_or_null,
                                                (const unsigned*)amaxy_or_null, part, st1, one);
            if (rc) return rc;
            return wgrad_reduce_launch(part, (int)sp, 1, C0, N, c_real, n_real, dw, part + (size_t)sp * C0 * N, st1);
        }
    }
    if (!take) return nbp_conv_wgrad_f32(src0, C0, src1, C1, ups, B, H, W, ksize, dy, N, c_real, n_real, dw, ws, ws_bytes, stream);
    NBP_RETURN_IF(c_real < 1 || c_real > C0 + C1 || n_real < 1 || n_real > N, NBP_E_ARG);
    int n_tiles, splits;
    wgrad_halo_plan(B, wide ? H : H / 2, wide ? W : W * 2, C0 + C1, N, &n_tiles, &splits);      // 64-pixel tiles either way
    NBP_RETURN_IF(ws_bytes < (size_t)splits * 9 * (C0 + C1) * N * sizeof(float) + 256 + 1024, NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    unsigned* amax3 = (unsigned*)(((uintptr_t)ws + 255) / 256 * 256);
    float* part = (float*)((char*)amax3 + 1024);
    int rc = nbp_wgrad_split_launch(src0, C0, src1, C1, ups, B, H, W, dy, N, n_tiles, splits, amax3, (const unsigned*)amax0_or_null,
                                    (const unsigned*)amax1_or_null, (const unsigned*)amaxy_or_null, part, st, one);
    if (rc) return rc;
    float* tmp = part + (size_t)splits * 9 * (C0 + C1) * N;
    const bool room = ws_bytes >= (size_t)(splits + WGRAD_REDUCE_GROUPS) * 9 * (C0 + C1) * N * sizeof(float) + 256 + 1024;
    return wgrad_reduce_launch(part, splits, 9, C0 + C1, N, c_real, n_real, dw, room ? tmp : nullptr, st);
}
extern "C" int nbp_conv_wgrad_split_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                                        int ksize, const float* dy, int N, int c_real, int n_real, float* dw,
                                        const void* amax0_or_null, const void* amax1_or_null, const void* amaxy_or_null, void* ws,
                                        size_t ws_bytes, void* stream) {
    NBP_ENTER();
    return conv_wgrad_split_impl(src0, C0, src1, C1, ups, B, H, W, ksize, dy, N, c_real, n_real, dw, amax0_or_null, amax1_or_null,
                                 amaxy_or_null, ws, ws_bytes, stream, 0);
}
// The one-piece form (wgrad_split_kernel / wgrad_1x1_split_kernel with ONE: hi = fp16(s x) alone, one MFMA per product) of the
// layers the split kernels take; the rest falls through to nbp_conv_wgrad_f32 exactly as above.
extern "C" int nbp_conv_wgrad_split_f32_h1(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                                           int ksize, const float* dy, int N, int c_real, int n_real, float* dw,
                                           const void* amax0_or_null, const void* amax1_or_null, const void* amaxy_or_null, void* ws,
                                           size_t ws_bytes, void* stream) {
    NBP_ENTER();
    return conv_wgrad_split_impl(src0, C0, src1, C1, ups, B, H, W, ksize, dy, N, c_real, n_real, dw, amax0_or_null, amax1_or_null,
                                 amaxy_or_null, ws, ws_bytes, stream, 1);
}

extern "C" int nbp_gather_values_f32(const float* out1_nchw, const long long* coords_bcxy, int K, int C, int H, int W, float* pred,
                                     void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(K < 0, NBP_E_ARG);
    if (K == 0) return 0;                                  // a batch without value targets is legal (empty gather)
    NBP_RETURN_IF(!out1_nchw || !coords_bcxy || !pred, NBP_E_ARG);
    gather_values_kernel<<<(unsigned)nbp_cdiv(K, 256), 256, 0, (hipStream_t)stream>>>(out1_nchw, coords_bcxy, K, C, H, W, pred);
    return nbp_launch_status();
}

extern "C" int nbp_scatter_values_f32(const float* dpred, const long long* coords_bcxy, int K, int C, int H, int W,
                                      float* dout1_nchw_zeroed, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(K < 0, NBP_E_ARG);
    if (K == 0) return 0;
    NBP_RETURN_IF(!dpred || !coords_bcxy || !dout1_nchw_zeroed, NBP_E_ARG);
    scatter_values_kernel<<<(unsigned)nbp_cdiv(K, 256), 256, 0, (hipStream_t)stream>>>(dpred, coords_bcxy, K, C, H, W,
                                                                                        dout1_nchw_zeroed);
    return nbp_launch_status();
}

// mode 0: MSE, mode 1: BCE.  *sum_out (device double) = sum of per-element losses; dp = coef * d(mean loss)/dp
extern "C" int nbp_loss_f32(int mode, const float* p, const float* t, long long n, float grad_coef, double* sum_out,
                            float* dp_or_null, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!p || !t || !sum_out || !ws || n < 1 || mode < 0 || mode > 1, NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < 512 * sizeof(double) + 256, NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)(((uintptr_t)ws + 255) / 256 * 256);
    const int nblk = nbp_ew_grid(n, 256) > 512 ? 512 : nbp_ew_grid(n, 256);
    loss_partial_kernel<<<nblk, 256, 0, st>>>(mode, p, t, n, part);
    int rc = nbp_launch_status();
    if (rc) return rc;
    sum_doubles_kernel<<<1, 64, 0, st>>>(part, nblk, sum_out);
    if ((rc = nbp_launch_status())) return rc;
    if (dp_or_null) {
        loss_grad_kernel<<<nbp_ew_grid(n, 256), 256, 0, st>>>(mode, p, t, n, grad_coef, dp_or_null);
        rc = nbp_launch_status();
    }
    return rc;
}
