// nbp_stat_rows.h -- the fixed-order statistics fold, once.  What makes a summary's float64 sums reproducible bit
// for bit is that nothing about their order is left to the hardware:
//   1. a fixed launch geometry of STAT_THREADS-thread blocks; every thread adds its strided elements in index order (the caller's
//      loop: the per-element work differs from summary to summary and stays with it);
//   2. stat_row_store: the threads of a block added by a fixed tree -- __shfl_down by 32, 16, ..., 1 inside a wave, lane 0 of each
//      wave to LDS, then waves 0..3 added in order by one thread -- and the block's row STORED (no floating-point atomics);
//   3. stat_rows_fold: a second small launch adds column `col` of the rows in index order.
// A row is NS float64 sums (their bits) followed by NC int64 counts, as 8-byte words; the rows' workspace is one carved buffer.
// Included inside each translation unit (anonymous namespace), like nbp_carve.h; tests/test_gpu_stat_rows.py pins the order.
#pragma once
#include "common.h"
#include "nbp_carve.h"

namespace {

constexpr int STAT_THREADS = 256, STAT_WAVES = STAT_THREADS / 64;

// The whole block calls this once with each thread's partials (sum[NS], cnt[NC]: clobbered); thread 0 stores the block's row.
template <int NS, int NC>
__device__ __forceinline__ void stat_row_store(double* sum, long long* cnt, unsigned long long* __restrict__ row) {
    __shared__ double wsum[STAT_WAVES][NS > 0 ? NS : 1];
    __shared__ long long wcnt[STAT_WAVES][NC > 0 ? NC : 1];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) sum[k] += __shfl_down(sum[k], off, 64);
#pragma unroll
        for (int k = 0; k < NC; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) wsum[wave][k] = sum[k];
#pragma unroll
        for (int k = 0; k < NC; ++k) wcnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < NS; ++k) {
            double s = wsum[0][k];
            for (int w = 1; w < STAT_WAVES; ++w) s += wsum[w][k];
            row[k] = (unsigned long long)__double_as_longlong(s);
        }
        for (int k = 0; k < NC; ++k) {
            long long s = 0;
            for (int w = 0; w < STAT_WAVES; ++w) s += wcnt[w][k];
            row[NS + k] = (unsigned long long)s;
        }
    }
}

// Column `col` of n_rows rows of row_words words, added in index order: a float64 sum's bits (col < n_sums) or a count.
__device__ __forceinline__ unsigned long long stat_rows_fold(const unsigned long long* __restrict__ rows, int n_rows, int row_words,
                                                             int n_sums, int col) {
    if (col < n_sums) {
        double s = 0.0;
        for (int b = 0; b < n_rows; ++b) s += __longlong_as_double((long long)rows[(size_t)b * row_words + col]);
        return (unsigned long long)__double_as_longlong(s);
    }
    long long s = 0;
    for (int b = 0; b < n_rows; ++b) s += (long long)rows[(size_t)b * row_words + col];
    return (unsigned long long)s;
}

// ---- host: the rows' workspace, n_rows rows of row_words words
unsigned long long* stat_rows_layout(Carver& c, size_t n_rows, int row_words) { return c.take<unsigned long long>(n_rows * (size_t)row_words); }
size_t stat_rows_bytes(size_t n_rows, int row_words) { return carved_bytes(0, stat_rows_layout, n_rows, row_words); }

}  // namespace
