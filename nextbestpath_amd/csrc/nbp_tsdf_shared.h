// nbp_tsdf_shared.h -- what the two files that read a TSDF volume share (nbp_tsdf.hip: integration, the fused cloud, statistics;
// nbp_tsdf_mesh.hip: the fused mesh): the volume's limits and geometry, the usable-voxel rule, a voxel's centre, the workgroup and
// run-offset scans of the count / scan / emit passes, and the host-side checks of a volume's arguments.
#pragma once
#include "common.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// fp32 with one rounding per operation, as the definitions have it: from here to the end of the including file (device code would
// otherwise fuse a multiply into the add behind it, across statements too)
#pragma clang fp contract(off)

namespace {

constexpr int TS_THREADS = 256;
constexpr long long TS_MAX_VOXELS = 1ll << 28;
constexpr int TS_QUANT = 127;
constexpr int EX_RUN = 2048;                        // consecutive voxels of one extraction workgroup: EX_RUN / TS_THREADS rounds

struct ExGeom { float lo[3]; float voxel; int nx, ny, nz; int min_weight; };

__device__ __forceinline__ float tsdf_centre(float lo, int i, float voxel) {
    const float s = ((float)i + 0.5f) * voxel;
    return lo + s;
}

__device__ __forceinline__ bool tsdf_usable(int2 sw, int min_weight) {
    const long long a = sw.x < 0 ? -(long long)sw.x : (long long)sw.x;
    return sw.y >= min_weight && a < (long long)TS_QUANT * sw.y;
}

// inclusive prefix sum of `x` over the workgroup's threads, in thread order (shuffles inside a wave, the four waves in order)
__device__ __forceinline__ int block_inclusive_scan(int x, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();                                                 // (the previous round's readers of wave_sums are done)
    if (lane == 63) wave_sums[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < TS_THREADS / 64; ++w) {
        const int s = wave_sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return x + before;
}

// one workgroup: runs[n_runs] -> exclusive offsets, in place; every thread gets the total.  wave_sums: TS_THREADS / 64 words of LDS
__device__ __forceinline__ long long scan_runs(long long* __restrict__ runs, long long n_runs, long long* wave_sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long long b0 = 0; b0 < n_runs; b0 += TS_THREADS) {
        const long long b = b0 + threadIdx.x;
        const long long own = b < n_runs ? runs[b] : 0;
        long long x = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        __syncthreads();
        if (lane == 63) wave_sums[wave] = x;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < TS_THREADS / 64; ++w) {
            const long long s = wave_sums[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (b < n_runs) runs[b] = carry + before + x - own;
        carry += all;
    }
    return carry;
}

// ---- host side
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// NBP_E_* of a volume's geometry, 0 when it is fine
int check_geometry(const void* vol, const float* lo, float voxel, int nx, int ny, int nz) {
    NBP_RETURN_IF(!vol || !lo || nx < 1 || ny < 1 || nz < 1, NBP_E_ARG);
    NBP_RETURN_IF(!(voxel > 0.f) || !isfinite(voxel) || !isfinite(lo[0]) || !isfinite(lo[1]) || !isfinite(lo[2]), NBP_E_ARG);
    NBP_RETURN_IF((long long)nx * ny > TS_MAX_VOXELS || (long long)nx * ny * nz > TS_MAX_VOXELS, NBP_E_SHAPE);
    NBP_RETURN_IF(((uintptr_t)vol & 7), NBP_E_SHAPE);
    return 0;
}

long long extract_runs(long long n_vox) { return nbp_cdiv(n_vox, EX_RUN); }

}  // namespace
