// nbp_replay.hip -- the compact replay record ("NBPC" version 1) on the device (include/nbp_hip.h: nbp_replay_encode_f32 /
// nbp_replay_decode_f32).  utility/replay_codec.py is the definition of the format; these kernels produce and consume its bytes.
//
// A stream holds the 6 planes of a record: a 64-byte header (magic, version, C, S, total_bytes, then {u32 nnz, u8 width, 3 zero
// bytes} per channel), then per channel a bitmap of S^2 / 8 bytes (bit k of 64-bit word g = row-major pixel 64 g + k, set where the
// fp32 bit pattern is not zero) and the non-zero pixels in row-major order at `width` bytes each, padded to 16.
//
// One workgroup per (record, channel), 64-pixel groups by wave: the ballot of a group IS its bitmap word, the group popcounts are
// scanned in LDS, and a value's place is its group's prefix plus its rank among the lanes below it.  No atomics, no workgroup waits
// for another: the order is fixed by construction.
//   encode   launch 1 (classify): nnz and width of every channel, written straight into the channel's header entry of its slot;
//            launch 2 (write): every workgroup sums the at most 5 section sizes in front of its own from those entries, writes its
//            bitmap and values; channel 0's also writes the first 16 header bytes.  Nothing beyond total_bytes is written.
//   decode   one launch: the header (validated by the host) gives the section offsets; nnz and width are clamped again here, and a
//            value index is clamped to nnz - 1, so no byte pattern moves a read out of nbp_replay_stream_bound(S) bytes behind the
//            stream's offset or a write out of the outputs.  Every output pixel is written, zeros included.
// The second read of a channel (the values pass) comes from the cache: a plane is 256 KB at S = 256.
#include "common.h"

namespace {

constexpr int RC = 6;                    // channels of a record
constexpr int HEADER = 16 + 8 * RC;
constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_S = 512;               // S^2 / 64 group counts in LDS
constexpr int MAX_GROUPS = MAX_S * MAX_S / 64;
constexpr int DECODE_BATCH = 64;         // stream offsets per launch (they ride in the kernel arguments)
constexpr unsigned ONE_BITS = 0x3F800000u;

__device__ __forceinline__ unsigned pad16(unsigned n) { return (n + 15u) & ~15u; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}

// what a non-zero pixel needs: bit 0 = not 1.0f, bit 1 = not an integer in [1, 255], bit 2 = not an integer in [1, 65535]
__device__ __forceinline__ int need_of(unsigned bits) {
    const float v = __uint_as_float(bits);
    int need = bits != ONE_BITS ? 1 : 0;
    const bool whole16 = v >= 1.0f && v <= 65535.0f && (float)(unsigned)v == v;      // false for NaN; the cast is in range
    if (!whole16) need |= 6;
    else if (v > 255.0f) need |= 2;
    return need;
}

__device__ __forceinline__ int width_of(int need) { return !need ? 0 : (need & 4) ? 4 : (need & 2) ? 2 : 1; }

// launch 1: grid = n * 6.  The channel's {nnz, width} into its header entry.
__global__ __launch_bounds__(THREADS) void replay_classify_kernel(const unsigned* __restrict__ rec, int SS, unsigned char* __restrict__ arena,
                                                                  size_t stride) {
    __shared__ int s_cnt[WAVES], s_need[WAVES];
    const int r = blockIdx.x / RC, c = blockIdx.x - r * RC;
    const uint4* __restrict__ src = (const uint4*)(rec + ((size_t)r * RC + c) * SS);
    int cnt = 0, need = 0;
    for (int q = threadIdx.x; q < SS / 4; q += THREADS) {
        const uint4 v = src[q];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w[k]) {
                ++cnt;
                need |= need_of(w[k]);
            }
    }
    cnt = wave_sum(cnt);
    need = wave_or(need);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_need[wave] = need;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0, m = 0;
        for (int w = 0; w < WAVES; ++w) {
            n += s_cnt[w];
            m |= s_need[w];
        }
        uint2 e;
        e.x = (unsigned)n;
        e.y = (unsigned)width_of(m);                    // u8 width + 3 zero bytes
        *(uint2*)(arena + (size_t)r * stride + 16 + 8 * c) = e;
    }
}

// Exclusive scan of cnt[0 .. G) in place by the whole workgroup (G <= MAX_GROUPS); every thread owns `per` consecutive entries.
__device__ __forceinline__ void scan_groups(int* cnt, int G, int* s_wave) {
    const int per = (G + THREADS - 1) / THREADS;
    const int lo = min((int)threadIdx.x * per, G), hi = min(lo + per, G);
    int sum = 0;
    for (int g = lo; g < hi; ++g) sum += cnt[g];
    int incl = sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    for (int g = lo; g < hi; ++g) {
        const int v = cnt[g];
        cnt[g] = base;
        base += v;
    }
    __syncthreads();
}

struct ChannelPlace {
    unsigned nnz, width, bitmap_off, value_off, total;
};

// The channel table of a header -> where channel c's sections lie.  nnz and width are clamped to what the format allows.
__device__ __forceinline__ ChannelPlace place_channel(const unsigned char* __restrict__ head, int c, int SS) {
    ChannelPlace p = {};
    unsigned pos = HEADER;
    for (int k = 0; k < RC; ++k) {
        const uint2 e = *(const uint2*)(head + 16 + 8 * k);
        const unsigned nnz = min(e.x, (unsigned)SS);
        unsigned width = e.y & 255u;
        if (width != 1 && width != 2 && width != 4) width = 0;
        if (k == c) {
            p.nnz = nnz;
            p.width = width;
            p.bitmap_off = pos;
            p.value_off = pos + SS / 8;
        }
        pos += SS / 8 + pad16(nnz * width);
    }
    p.total = pos;
    return p;
}

// launch 2: grid = n * 6.
__global__ __launch_bounds__(THREADS) void replay_write_kernel(const unsigned* __restrict__ rec, int S, unsigned char* __restrict__ arena,
                                                               size_t stride) {
    __shared__ int s_pre[MAX_GROUPS];
    __shared__ int s_wave[WAVES];
    const int SS = S * S, G = SS / 64;
    const int r = blockIdx.x / RC, c = blockIdx.x - r * RC;
    const unsigned* __restrict__ src = rec + ((size_t)r * RC + c) * SS;
    unsigned char* slot = arena + (size_t)r * stride;
    const ChannelPlace p = place_channel(slot, c, SS);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (c == 0 && threadIdx.x == 0) {
        uint4 h;
        h.x = 0x4350424Eu;                               // "NBPC"
        h.y = 1u | ((unsigned)RC << 16);                 // u16 version, u16 C
        h.z = (unsigned)S;
        h.w = p.total;
        *(uint4*)slot = h;
    }
    unsigned long long* bitmap = (unsigned long long*)(slot + p.bitmap_off);
    for (int g = wave; g < G; g += WAVES) {
        const unsigned long long mask = __ballot(src[(size_t)g * 64 + lane] != 0u);
        if (lane == 0) {
            bitmap[g] = mask;
            s_pre[g] = __popcll(mask);
        }
    }
    if (p.width == 0) return;                            // (uniform over the workgroup)
    __syncthreads();
    scan_groups(s_pre, G, s_wave);
    unsigned char* vals = slot + p.value_off;
    for (int g = wave; g < G; g += WAVES) {
        const unsigned bits = src[(size_t)g * 64 + lane];
        const unsigned long long mask = __ballot(bits != 0u);
        if (bits != 0u) {
            const unsigned at = (unsigned)s_pre[g] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            if (p.width == 4) ((unsigned*)vals)[at] = bits;
            else if (p.width == 2) ((unsigned short*)vals)[at] = (unsigned short)(unsigned)__uint_as_float(bits);
            else vals[at] = (unsigned char)(unsigned)__uint_as_float(bits);
        }
    }
    const unsigned used = p.nnz * p.width, pad = pad16(used) - used;
    if (threadIdx.x < pad) vals[used + threadIdx.x] = 0;
}

struct DecodeOffsets {
    long long at[DECODE_BATCH];
};

// grid = n * 6 (n <= DECODE_BATCH).  Channel c of record r into x_out [n,5,S,S] (c < 5) or gt_out [n,1,S,S].
__global__ __launch_bounds__(THREADS) void replay_decode_kernel(const unsigned char* __restrict__ streams, DecodeOffsets offs, int S,
                                                                unsigned* __restrict__ x_out, unsigned* __restrict__ gt_out) {
    __shared__ int s_pre[MAX_GROUPS];
    __shared__ int s_wave[WAVES];
    const int SS = S * S, G = SS / 64;
    const int r = blockIdx.x / RC, c = blockIdx.x - r * RC;
    const unsigned char* __restrict__ st = streams + offs.at[r];
    const ChannelPlace p = place_channel(st, c, SS);
    unsigned* __restrict__ dst = c < 5 ? x_out + ((size_t)r * 5 + c) * SS : gt_out + (size_t)r * SS;
    const unsigned long long* __restrict__ bitmap = (const unsigned long long*)(st + p.bitmap_off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool values = p.width != 0 && p.nnz != 0;
    if (values) {
        for (int g = threadIdx.x; g < G; g += THREADS) s_pre[g] = __popcll(bitmap[g]);
        __syncthreads();
        scan_groups(s_pre, G, s_wave);
    }
    const unsigned char* __restrict__ vals = st + p.value_off;
    for (int g = wave; g < G; g += WAVES) {
        const unsigned long long mask = bitmap[g];
        unsigned bits = 0u;
        if ((mask >> lane) & 1ull) {
            if (!values) {
                bits = p.width == 0 ? ONE_BITS : 0u;     // (width != 0 with nnz == 0: a bitmap the header contradicts decodes to zeros)
            } else {
                const unsigned at = min((unsigned)s_pre[g] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull)), p.nnz - 1u);
                if (p.width == 4) bits = ((const unsigned*)vals)[at];
                else if (p.width == 2) bits = __float_as_uint((float)((const unsigned short*)vals)[at]);
                else bits = __float_as_uint((float)vals[at]);
            }
        }
        dst[(size_t)g * 64 + lane] = bits;
    }
}

bool replay_side_ok(int S) { return S >= 16 && S <= MAX_S && S % 16 == 0; }

}  // namespace

extern "C" size_t nbp_replay_stream_bound(int S) {
    if (!replay_side_ok(S)) return 0;
    const size_t SS = (size_t)S * S;
    return HEADER + RC * (SS / 8 + 4 * SS);
}

extern "C" int nbp_replay_encode_f32(const float* rec, int n, int S, void* arena, size_t stride_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!rec || !arena || n < 1, NBP_E_ARG);
    NBP_RETURN_IF(!replay_side_ok(S) || (long long)n * RC > 0x7fffffffll, NBP_E_SHAPE);
    NBP_RETURN_IF(stride_bytes < nbp_replay_stream_bound(S) || stride_bytes % 16 != 0, NBP_E_WS);
    NBP_RETURN_IF((((uintptr_t)rec | (uintptr_t)arena) & 15) != 0, NBP_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    replay_classify_kernel<<<n * RC, THREADS, 0, st>>>((const unsigned*)rec, S * S, (unsigned char*)arena, stride_bytes);
    replay_write_kernel<<<n * RC, THREADS, 0, st>>>((const unsigned*)rec, S, (unsigned char*)arena, stride_bytes);
    return nbp_launch_status();
}

extern "C" int nbp_replay_decode_f32(const void* streams, const long long* offsets_host, int n, int S, float* x_out, float* gt_out,
                                     void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!streams || !offsets_host || !x_out || !gt_out || n < 1, NBP_E_ARG);
    NBP_RETURN_IF(!replay_side_ok(S), NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)streams | (uintptr_t)x_out | (uintptr_t)gt_out) & 15) != 0, NBP_E_SHAPE);
    for (int r = 0; r < n; ++r) NBP_RETURN_IF(offsets_host[r] < 0 || offsets_host[r] % 16 != 0, NBP_E_ARG);
    const size_t SS = (size_t)S * S;
    for (int r0 = 0; r0 < n; r0 += DECODE_BATCH) {
        const int m = n - r0 < DECODE_BATCH ? n - r0 : DECODE_BATCH;
        DecodeOffsets offs = {};
        for (int r = 0; r < m; ++r) offs.at[r] = offsets_host[r0 + r];
        replay_decode_kernel<<<m * RC, THREADS, 0, (hipStream_t)stream>>>((const unsigned char*)streams, offs, S,
                                                                          (unsigned*)x_out + (size_t)r0 * 5 * SS,
                                                                          (unsigned*)gt_out + (size_t)r0 * SS);
    }
    return nbp_launch_status();
}
