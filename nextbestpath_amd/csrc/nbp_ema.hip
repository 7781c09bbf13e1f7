// nbp_ema.hip -- exponential moving average of a set of fp32 tensors (the weights and BatchNorm statistics of the network under
// training), updated on the device behind the optimizer step (include/nbp_hip.h: nbp_ema_update_f32).
//
// Work distribution: nbp_multi_tensor.h (the tables of nbp_optim.hip): one record {p, e, numel} per tensor, one 16384-element
// chunk per workgroup of 256 threads, 16-byte accesses where both addresses allow them.  12 bytes per element: p and e read, e
// written.
//
// Per element, with d the decay of this update:  e' = fl32(d e + (1 - d) p), evaluated in double from the fp32 operands and
// rounded once (the choice adamw_kernel makes for m': the pass is bound by its traffic, the fp64 rate is nowhere near it).  This
// association of e + (1 - d)(p - e) is a copy at d = 0 whatever the operands are (p - e alone can lose a p that is 2^-30 of e).
//
// d is formed on the device from `num_updates` (n), an integer in the 16-byte state block: warm-up on, d = min(decay, (1 + n) /
// (10 + n)) in double (an integer quotient, then min: the same bits as the host's expression); off, d = decay.
//
// Gate: with the state block of a HipAdamW given, an update whose optimizer step was dropped (applied = 0) returns before its
// first load: e and n keep their bits.  Stream order behind the optimizer's finalize launch makes `applied` valid.
//
// Counter: every workgroup of the update launch READS n; a one-thread launch behind it on the same stream writes n + 1 (under
// the same gate).  No workgroup of one launch both reads and writes it, so there is nothing to race; no atomics, no hand-off
// between workgroups.
#include "common.h"
#include "nbp_multi_tensor.h"

#include <stddef.h>

namespace {

struct EmaDesc {                                 // nbp_ema_desc_bytes() = 24
    const float* p;
    float* e;
    long long numel;
};
struct EmaState {                                // nbp_ema_state_bytes() = 16
    int num_updates;
    int pad[3];
};

static_assert(sizeof(EmaDesc) == 24 && sizeof(EmaState) == 16, "table layouts are part of the ABI");

__device__ __forceinline__ float ema_avg(double d, double omd, float e, float p) {
    return (float)fma(d, (double)e, omd * (double)p);
}

__global__ __launch_bounds__(OPT_THREADS) void ema_kernel(const EmaDesc* __restrict__ descs, const OptChunk* __restrict__ chunks,
                                                           const EmaState* __restrict__ state, const OptState* __restrict__ gate,
                                                           double decay, int warmup) {
    if (gate && !gate->applied) return;                            // the optimizer dropped its step: e keeps its bits
    const OptChunk ck = chunks[blockIdx.x];
    const EmaDesc t = descs[ck.tensor];
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.e) & 15) == 0);
    const int tid = threadIdx.x;
    double d = decay;
    if (warmup) {
        const double n = (double)state->num_updates;
        const double w = (1.0 + n) / (10.0 + n);
        d = w < decay ? w : decay;
    }
    const double omd = 1.0 - d;
    if (vec && t.numel - ck.first >= OPT_CHUNK) {
        // a whole chunk of aligned quads (3 044 of the network's 3 295 chunks): a loop of its own, so that its 16-byte
        // stores stay whole (sharing a loop with the tail path, the compiler merges the quad's last store with the tail's)
        const float4* __restrict__ p4 = (const float4*)(t.p + ck.first);
        float4* __restrict__ e4 = (float4*)(t.e + ck.first);
#pragma unroll 4
        for (int i = 0; i < OPT_QUADS; ++i) {
            const int q = i * OPT_THREADS + tid;
            const float4 p = p4[q];
            float4 e = e4[q];
            e.x = ema_avg(d, omd, e.x, p.x);
            e.y = ema_avg(d, omd, e.y, p.y);
            e.z = ema_avg(d, omd, e.z, p.z);
            e.w = ema_avg(d, omd, e.w, p.w);
            e4[q] = e;
        }
        return;
    }
#pragma unroll 4
    for (int i = 0; i < OPT_QUADS; ++i) {                          // a tensor's last chunk, or a tensor off the 16-byte grid
        const long long el = ck.first + 4ll * (i * OPT_THREADS + tid);
        const long long left = t.numel - el;
        if (left <= 0) break;
        const int cnt = left < 4 ? (int)left : 4;
        float p[4], e[4];
        load_quad(t.p, el, cnt, vec, p);
        load_quad(t.e, el, cnt, vec, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = ema_avg(d, omd, e[k], p[k]);
        store_quad(t.e, el, cnt, vec, e);
    }
}

// One thread, behind ema_kernel on the stream.
__global__ void ema_tick_kernel(EmaState* __restrict__ state, const OptState* __restrict__ gate) {
    if (gate && !gate->applied) return;
    state->num_updates += 1;
}

}  // namespace

extern "C" int nbp_ema_desc_bytes(void) { return (int)sizeof(EmaDesc); }
extern "C" size_t nbp_ema_state_bytes(void) { return sizeof(EmaState); }

extern "C" int nbp_ema_update_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, void* ema_state,
                                  const void* optim_state_or_null, double decay, int warmup, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!descs_dev || !chunks_dev || !ema_state || n_chunks < 1, NBP_E_ARG);
    NBP_RETURN_IF(!(decay >= 0.0 && decay < 1.0), NBP_E_ARG);
    ema_kernel<<<dim3((unsigned)n_chunks), OPT_THREADS, 0, (hipStream_t)stream>>>((const EmaDesc*)descs_dev, (const OptChunk*)chunks_dev,
                                                                                 (const EmaState*)ema_state, (const OptState*)optim_state_or_null,
                                                                                 decay, warmup ? 1 : 0);
    ema_tick_kernel<<<dim3(1), 1, 0, (hipStream_t)stream>>>((EmaState*)ema_state, (const OptState*)optim_state_or_null);
    return nbp_launch_status();
}
