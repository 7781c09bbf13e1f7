// Probe (GPU box): a latency-bound filler kernel with a chosen register and LDS footprint, to run beside the split forward
// (tools/diag/slack_probe.py).  The question: does a 256-thread workgroup of <= 32 VGPRs and <= 16 KB of LDS fit beside two
// resident convolution workgroups (2 x 240 of a SIMD's 512 registers, 2 x 64..70 of a CU's 160 KB) where a heavier one takes the
// place of one of them?
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -Rpass-analysis=kernel-resource-usage tools/probes/slack_probe.hip \
//         -o tools/probes/libslack_probe.so
// LIVE is the number of values kept live across the loop, not the register count: the allocation is what the remark prints
// (slack_probe.py prints that table next to the timings).
#include <hip/hip_runtime.h>

namespace {

// One workgroup per CU and launch; every lane chases its own chain of `iters` dependent loads through `ring` (n entries, n a power
// of two; the index is masked, so no content of the ring can take a load outside it).
template <int LIVE, int LDS_BYTES>
__global__ __launch_bounds__(256) void slack_filler_kernel(const unsigned* __restrict__ ring, unsigned mask, int iters,
                                                           unsigned* __restrict__ out) {
    unsigned acc[LIVE];
#pragma unroll
    for (int u = 0; u < LIVE; ++u) acc[u] = threadIdx.x * 2654435761u + (unsigned)u;
    unsigned idx = (blockIdx.x * 256u + threadIdx.x) * 2246822519u & mask;
    if constexpr (LDS_BYTES > 0) {
        __shared__ unsigned lds[LDS_BYTES / 4];
        for (int i = threadIdx.x; i < LDS_BYTES / 4; i += 256) lds[i] = i ^ idx;
        __syncthreads();
        idx = (idx + lds[(threadIdx.x * 97u) % (LDS_BYTES / 4)]) & mask;
    }
    for (int it = 0; it < iters; ++it) {
        idx = ring[idx] & mask;
#pragma unroll
        for (int u = 0; u < LIVE; ++u) acc[u] = acc[u] * 1664525u + (idx ^ (unsigned)u);
    }
    unsigned s = idx;
#pragma unroll
    for (int u = 0; u < LIVE; ++u) s ^= acc[u];
    out[blockIdx.x * 256u + threadIdx.x] = s;
}

template <int LIVE, int LDS_BYTES>
int launch(const unsigned* ring, unsigned mask, int iters, unsigned* out, int blocks, hipStream_t st) {
    slack_filler_kernel<LIVE, LDS_BYTES><<<blocks, 256, 0, st>>>(ring, mask, iters, out);
    return (int)hipGetLastError();
}

}  // namespace

// regs: the footprint aimed at (24, 32, 40, 48, 56 or 64 allocated VGPRs); lds_kb: 0, 16 or 24.  `ring` holds n = mask + 1 entries, `out` blocks * 256.
#define SLACK_LIVE_24 16
#define SLACK_LIVE_32 24
#define SLACK_LIVE_40 32
#define SLACK_LIVE_48 40
#define SLACK_LIVE_56 48
#define SLACK_LIVE_64 56
extern "C" int slack_filler_launch(int regs, int lds_kb, const unsigned* ring, unsigned n, int iters, unsigned* out, int blocks,
                                   void* stream) {
    if (!ring || !out || n == 0 || (n & (n - 1)) || iters < 0 || iters > 4096 || blocks < 1) return -1;
    hipStream_t st = (hipStream_t)stream;
    const unsigned mask = n - 1;
#define SLACK_CASE(R, LIVE)                                                                               \
    if (regs == R) {                                                                                      \
        if (lds_kb == 0) return launch<LIVE, 0>(ring, mask, iters, out, blocks, st);                      \
        if (lds_kb == 16) return launch<LIVE, 16 * 1024>(ring, mask, iters, out, blocks, st);             \
        if (lds_kb == 24) return launch<LIVE, 24 * 1024>(ring, mask, iters, out, blocks, st);             \
        return -1;                                                                                        \
    }
    SLACK_CASE(24, SLACK_LIVE_24)
    SLACK_CASE(32, SLACK_LIVE_32)
    SLACK_CASE(40, SLACK_LIVE_40)
    SLACK_CASE(48, SLACK_LIVE_48)
    SLACK_CASE(56, SLACK_LIVE_56)
    SLACK_CASE(64, SLACK_LIVE_64)
#undef SLACK_CASE
    return -1;
}
