// nbp_optim.hip -- multi-tensor AdamW with device-side gradient-norm clipping and non-finite step skipping
// (include/nbp_hip.h: nbp_grad_sqnorm_f32, nbp_optim_finalize_f32, nbp_adamw_f32).
//
// The parameters stay where torch allocated them: a device table holds one record {p, g, m, v, numel} per tensor and a second
// table cuts every tensor into chunks of OPT_CHUNK elements, one workgroup per chunk (the idiom of nbp_prepack_weights_split:
// the launch reads its work from tables the caller built once).  Three kernels:
//   grad_sqnorm   one double per chunk: the sum of g^2 over the chunk, every product and every addition in double, in an order
//                 fixed by the element's position alone (lane = quad % 256, quads of a lane in ascending order, then the wave's
//                 xor tree, then the four waves through LDS in wave order).  No atomics, no hand-off between workgroups.
//   finalize      one workgroup: adds the partials in a fixed order in double and writes the state block -- norm, clip
//                 coefficient, finite flag, step counter, the bias corrections of every param group, the skipped-step count --
//                 and the per-parameter `step` scalars of the optimizer's state_dict.
//   adamw         the update of one param group; reads the step-dependent scalars from the state block, so the host never
//                 needs a value from the device.  Writes nothing when the step is skipped.
//
// Arithmetic of the update, per element (u = 2^-24): g^ = coef * g, m' and v' are evaluated in double from the fp32 operands
// and rounded once (|m' - m_exact| <= u |m'| plus the fp32 rounding of coef; double products of fp32 values are exact), the
// parameter in fp32: p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps).  The double work is ~11 operations per
// element beside 28 bytes of traffic: it hides under the memory time.
//
// Memory access: a lane moves quads (16 bytes) of p, g, m, v; a tensor whose four base addresses are not all 16-byte aligned
// takes the same element-to-lane assignment with 4-byte accesses, so results do not depend on alignment.  The last numel % 4
// elements of a tensor are a partial quad of one lane.
#include "common.h"
#include "nbp_multi_tensor.h"

#include <math.h>
#include <stddef.h>

namespace {

struct OptDesc {                                 // nbp_optim_desc_bytes() = 40
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
};
struct OptBetas {
    double b1[OPT_MAX_GROUPS], b2[OPT_MAX_GROUPS];
};

static_assert(sizeof(OptDesc) == 40, "table layouts are part of the ABI");

__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_kernel(const OptDesc* __restrict__ descs, const OptChunk* __restrict__ chunks,
                                                                   double* __restrict__ partial) {
    __shared__ double wave_sum[OPT_THREADS / 64];
    const OptChunk ck = chunks[blockIdx.x];
    const OptDesc d = descs[ck.tensor];
    const bool vec = ((uintptr_t)d.g & 15) == 0;
    const int tid = threadIdx.x;
    double acc = 0.0;
#pragma unroll 4
    for (int i = 0; i < OPT_QUADS; ++i) {
        const long long e = ck.first + 4ll * (i * OPT_THREADS + tid);
        const long long left = d.numel - e;
        if (left <= 0) break;
        float g[4];
        load_quad(d.g, e, left < 4 ? (int)left : 4, vec, g);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fma((double)g[k], (double)g[k], acc);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = wave_sum[0];
#pragma unroll
        for (int w = 1; w < OPT_THREADS / 64; ++w) s += wave_sum[w];
        partial[blockIdx.x] = s;
    }
}

// One workgroup.  partial == nullptr: the norm pass did not run (no clipping, no skipping): the step is applied with coef 1.
__global__ __launch_bounds__(OPT_THREADS) void optim_finalize_kernel(const double* __restrict__ partial, int n_partial, double max_norm,
                                                                      int skip_nonfinite, OptBetas betas, int n_groups,
                                                                      OptState* __restrict__ state, float* __restrict__ steps, int n_steps) {
    __shared__ double seg[OPT_THREADS];
    __shared__ float new_step;
    __shared__ int apply;
    const int tid = threadIdx.x;
    if (partial) {               // thread t: its contiguous run of partials in index order; thread 0: the 256 runs in index order
        const int per = (n_partial + OPT_THREADS - 1) / OPT_THREADS;
        const int lo = tid * per, hi = min(lo + per, n_partial);
        double s = 0.0;
        for (int i = lo; i < hi; ++i) s += partial[i];
        seg[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float norm = 0.0f, coef = 1.0f;
        int finite = 1;
        if (partial) {
            double s = 0.0;
            for (int i = 0; i < OPT_THREADS; ++i) s += seg[i];
            const double nrm = sqrt(s);
            finite = isfinite(s) ? 1 : 0;          // g^2 cannot overflow a double: s is non-finite iff some gradient element is
            norm = (float)nrm;
            if (max_norm > 0.0) {                  // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1); a NaN stays a NaN
                const double c = max_norm / (nrm + 1e-6);
                coef = c != c ? (float)c : (c < 1.0 ? (float)c : 1.0f);
            }
        }
        const int ap = (skip_nonfinite && !finite) ? 0 : 1;
        const float st = state->step + (ap ? 1.0f : 0.0f);
        state->total_norm = norm;
        state->clip_coef = coef;
        state->finite = finite;
        state->applied = ap;
        state->step = st;
        if (!ap) state->skipped_steps += 1;
        if (ap)
            for (int gi = 0; gi < n_groups; ++gi) {
                state->bc[2 * gi] = (float)(1.0 - pow(betas.b1[gi], (double)st));
                state->bc[2 * gi + 1] = (float)sqrt(1.0 - pow(betas.b2[gi], (double)st));
            }
        new_step = st;
        apply = ap;
    }
    __syncthreads();
    if (apply)
        for (int i = tid; i < n_steps; i += OPT_THREADS) steps[i] = new_step;
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(const OptDesc* __restrict__ descs, const OptChunk* __restrict__ chunks,
                                                             const OptState* __restrict__ state, int group, double lr, double beta1,
                                                             double beta2, double eps, double weight_decay) {
    if (!state->applied) return;                                   // a skipped step: p, m, v stay bit for bit
    const OptChunk ck = chunks[blockIdx.x];
    const OptDesc d = descs[ck.tensor];
    const bool vec = ((((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.m | (uintptr_t)d.v) & 15) == 0);
    const int tid = threadIdx.x;
    const double coef = (double)state->clip_coef;                  // exactly 1 without clipping: g^ = g bit for bit
    const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
    const float decay = (float)(1.0 - lr * weight_decay);
    const float step_size = (float)(lr / (double)state->bc[2 * group]);
    const float sqrt_bc2 = state->bc[2 * group + 1];
    const float epsf = (float)eps;
#pragma unroll 4
    for (int i = 0; i < OPT_QUADS; ++i) {
        const long long e = ck.first + 4ll * (i * OPT_THREADS + tid);
        const long long left = d.numel - e;
        if (left <= 0) break;
        const int cnt = left < 4 ? (int)left : 4;
        float p[4], g[4], m[4], v[4];
        load_quad(d.p, e, cnt, vec, p);
        load_quad(d.g, e, cnt, vec, g);
        load_quad(d.m, e, cnt, vec, m);
        load_quad(d.v, e, cnt, vec, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double gh = coef * (double)g[k];                 // exact: 24 x 24 bits
            const float mn = (float)fma(beta1, (double)m[k], omb1 * gh);
            const float vn = (float)fma(beta2, (double)v[k], omb2 * (gh * gh));
            const float denom = sqrtf(vn) / sqrt_bc2 + epsf;
            p[k] = p[k] * decay - step_size * (mn / denom);
            m[k] = mn;
            v[k] = vn;
        }
        store_quad(d.p, e, cnt, vec, p);
        store_quad(d.m, e, cnt, vec, m);
        store_quad(d.v, e, cnt, vec, v);
    }
}

}  // namespace

extern "C" int nbp_optim_desc_bytes(void) { return (int)sizeof(OptDesc); }
extern "C" int nbp_optim_chunk_elems(void) { return OPT_CHUNK; }
extern "C" size_t nbp_optim_workspace_bytes(long long n_chunks) { return n_chunks < 1 ? 0 : (size_t)n_chunks * sizeof(double); }
extern "C" size_t nbp_optim_state_bytes(int n_groups) {
    return (n_groups < 1 || n_groups > OPT_MAX_GROUPS) ? 0 : offsetof(OptState, bc) + 2 * sizeof(float) * (size_t)n_groups;
}

extern "C" int nbp_grad_sqnorm_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!descs_dev || !chunks_dev || !ws || n_chunks < 1, NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_optim_workspace_bytes(n_chunks), NBP_E_WS);
    grad_sqnorm_kernel<<<dim3((unsigned)n_chunks), OPT_THREADS, 0, (hipStream_t)stream>>>((const OptDesc*)descs_dev, (const OptChunk*)chunks_dev,
                                                                                         (double*)ws);
    return nbp_launch_status();
}

extern "C" int nbp_optim_finalize_f32(const void* ws_or_null, int n_chunks, double max_norm, int skip_nonfinite, const double* betas_host,
                                      int n_groups, void* state, void* steps_or_null, int n_steps, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!state || !betas_host || n_groups < 1 || n_groups > OPT_MAX_GROUPS || n_steps < 0 || (n_steps > 0 && !steps_or_null), NBP_E_ARG);
    NBP_RETURN_IF(ws_or_null && n_chunks < 1, NBP_E_ARG);
    NBP_RETURN_IF(!ws_or_null && (max_norm > 0.0 || skip_nonfinite), NBP_E_ARG);      // clipping and skipping need the norm pass
    NBP_RETURN_IF(max_norm != max_norm, NBP_E_ARG);
    OptBetas b = {};
    for (int i = 0; i < n_groups; ++i) {
        b.b1[i] = betas_host[2 * i];
        b.b2[i] = betas_host[2 * i + 1];
        NBP_RETURN_IF(!(b.b1[i] >= 0.0 && b.b1[i] < 1.0 && b.b2[i] >= 0.0 && b.b2[i] < 1.0), NBP_E_ARG);
    }
    optim_finalize_kernel<<<dim3(1), OPT_THREADS, 0, (hipStream_t)stream>>>((const double*)ws_or_null, n_chunks, max_norm, skip_nonfinite ? 1 : 0, b,
                                                                           n_groups, (OptState*)state, (float*)steps_or_null, n_steps);
    return nbp_launch_status();
}

extern "C" int nbp_adamw_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, const void* state, int group, double lr,
                             double beta1, double beta2, double eps, double weight_decay, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!descs_dev || !chunks_dev || !state || n_chunks < 1 || group < 0 || group >= OPT_MAX_GROUPS, NBP_E_ARG);
    adamw_kernel<<<dim3((unsigned)n_chunks), OPT_THREADS, 0, (hipStream_t)stream>>>((const OptDesc*)descs_dev, (const OptChunk*)chunks_dev,
                                                                                   (const OptState*)state, group, lr, beta1, beta2, eps,
                                                                                   weight_decay);
    return nbp_launch_status();
}
