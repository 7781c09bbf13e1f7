// nbp_multi_tensor.h -- what the multi-tensor kernels share (nbp_optim.hip: AdamW; nbp_ema.hip: the weight average).
//
// The tensors stay where torch allocated them.  A launch reads its work from two device tables the caller built once: one record
// per tensor (each kernel family has its own record type) and one OptChunk per workgroup, which names a tensor and the first of
// its OPT_CHUNK elements the workgroup moves.  Lane t of the workgroup moves quads t, t + 256, ... of the chunk; a tensor whose
// base addresses are not all 16-byte aligned takes the same element-to-lane assignment with 4-byte accesses, so results do not
// depend on alignment, and the last numel % 4 elements of a tensor are a partial quad of one lane.
#pragma once
#include "common.h"

namespace {

constexpr int OPT_CHUNK = 16384;                 // elements per workgroup: 16 quads per lane
constexpr int OPT_THREADS = 256;
constexpr int OPT_QUADS = OPT_CHUNK / (4 * OPT_THREADS);
constexpr int OPT_MAX_GROUPS = 16;

struct OptChunk {                                // 16 bytes
    long long first;                             // first element of the chunk inside its tensor (a multiple of OPT_CHUNK)
    int tensor;
    int pad;
};
struct OptState {                                // nbp_optim_state_bytes(n_groups) = 32 + 8 n_groups
    float total_norm;
    float clip_coef;
    int finite;
    int applied;                                 // 1: this step's update runs, 0: it is skipped
    float step;
    int skipped_steps;
    int pad[2];
    float bc[2 * OPT_MAX_GROUPS];                // per param group: 1 - beta1^step, sqrt(1 - beta2^step)   (only n_groups pairs exist)
};

static_assert(sizeof(OptChunk) == 16, "table layouts are part of the ABI");

__device__ __forceinline__ void load_quad(const float* __restrict__ base, long long e, int cnt, bool vec, float (&o)[4]) {
    if (vec && cnt == 4) {
        const float4 t = *(const float4*)(base + e);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < cnt ? base[e + k] : 0.0f;
    }
}

__device__ __forceinline__ void store_quad(float* __restrict__ base, long long e, int cnt, bool vec, const float (&o)[4]) {
    if (vec && cnt == 4) {
        *(float4*)(base + e) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) base[e + k] = o[k];
    }
}

}  // namespace
