// nbp_shell_walk.h -- the device side of the shell-walk grids (the host side: nbp_nn_grid.h): the reach and in-box tests, the
// device-count clamp, the walk over the shells of cells around a query and the query kernel on top of it, shared by the
// nearest-neighbour plan (nbp_recon.hip: cells of sorted points) and the triangle plan (nbp_surface.hip: cells of triangle entries).
// Included inside each translation unit; not part of the C ABI.
//
// The walk.  LANES lanes per query walk the shells of cells at Chebyshev cell distance r = r0, ..., R = ceil(cap / w) around the
// query's UNCLAMPED cell.  k is the fastest cell index, so the z cells of an (x, y) column are one contiguous run of the plan's
// payload: a column on the rim of the shell's square is one run over its 2 r + 1 cells (two loads of `start`), a column inside the
// square contributes its two end cells.  What a run holds, and what its distance to the query is, is the caller's `run`.
//
// Why the walk may stop after shell r once best <= fl(r w)^2, and after shell R whatever it found.  Cells are 1.001 w wide.  A
// target in a cell that shells 0..r do not hold differs from the query's cell by at least r + 1 on some axis, so their cell
// coordinates u = fl(fl(x - lo) inv) differ by more than r there.  u carries a relative error below 2^-23, i.e. below n 2^-23
// cells on an axis of n cells; with n <= NN_MAX_AXIS = 2048 (more is NBP_E_SHAPE) the two errors together stay below 0.0005 cells
// (plus r 2^-23 for a query r cells outside the grid), so for r >= 1 the real separation on that axis exceeds (r - 0.0005) 1.001 w
// > r w by a margin of 4e-4 relative, which dwarfs the 2^-24 roundings of e = fl(t - q), fl(e e) and fl(r w).  Rounding is
// monotone, so the pair's fp32 squared distance
// ((ex ex + ey ey) + ez ez) >= fl(e e) > fl(r w)^2 >= best: it cannot lower the minimum.  (r = 0: best <= 0 is a minimum already.)
// After shell R every unvisited target is farther than R w >= cap: its squared distance exceeds cap2.  So the result is the
// brute-force minimum over all targets of the plan, bit for bit.  A `run` whose targets are not points says in its own file what
// stands for "target" here (nbp_surface.hip: the nearest point of a triangle's box).  No atomics touch the output.
#pragma once
#include "nbp_nn_grid.h"

#pragma clang fp contract(off)                   // (the including files' bits are pinned with it: it must cover this header's code)

namespace {

// The device's count if there is one, clamped to the host's bound: rows at or beyond it are never read or written.
__device__ __forceinline__ long long dev_count(const long long* __restrict__ n_dev, long long n_host) {
    const long long n = n_dev ? *n_dev : n_host;
    return n < 0 ? 0 : (n > n_host ? n_host : n);
}

// lo <= p <= hi in fp32: a NaN is outside
__device__ __forceinline__ bool in_box(const Grid& g, const Box& bx, float x, float y, float z) {
    return x >= g.lo[0] && x <= bx.hi[0] && y >= g.lo[1] && y <= bx.hi[1] && z >= g.lo[2] && z <= bx.hi[2];
}

// Is the point's unclamped cell within R cells of the grid?  Then c gets that cell (otherwise c is not written).
__device__ __forceinline__ bool cell_in_reach(const Grid& g, int R, float x, float y, float z, int* c) {
    // the unclamped cell, clamped as a FLOAT to one cell beyond the reach of R before the conversion (a query 1e6 away, or a
    // NaN, must not reach the int conversion's undefined range)
    const float fi = floorf((x - g.lo[0]) * g.inv), fj = floorf((y - g.lo[1]) * g.inv), fk = floorf((z - g.lo[2]) * g.inv);
    const bool reach = fi >= (float)-R && fi <= (float)(g.n[0] - 1 + R) && fj >= (float)-R && fj <= (float)(g.n[1] - 1 + R) &&
                       fk >= (float)-R && fk <= (float)(g.n[2] - 1 + R);
    if (reach) { c[0] = (int)fi; c[1] = (int)fj; c[2] = (int)fk; }
    return reach;
}

// The minimum of the query's LANES lanes, in all of them.
template <int LANES>
__device__ __forceinline__ float lanes_min(float best) {
#pragma unroll
    for (int o = LANES / 2; o; o >>= 1) {
        const float other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    return best;
}

// The truncated minimum over the plan's targets for the query (x, y, z), reached by the query's LANES lanes together (lane `sub`
// of them); run(p, hi, best) -> best lowers best by the targets of payload slots [p, hi).  A query beyond reach, or with a NaN,
// gets cap2 without a memory access.
template <int LANES, class Run>
__device__ __forceinline__ float shell_walk(const Grid& g, int R, float w, float cap2, const int* __restrict__ start, int sub, float x,
                                            float y, float z, Run run) {
    const int n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    float best = cap2;
    int c[3];
    if (!cell_in_reach(g, R, x, y, z, c)) return best;             // (uniform over the query's lanes)
    const int ci = c[0], cj = c[1], ck = c[2];
    // shells closer than the grid hold no cell: a query outside starts at its Chebyshev cell distance to the grid (<= R)
    const int r0 = max(max(max(-ci, ci - (n0 - 1)), max(-cj, cj - (n1 - 1))), max(max(-ck, ck - (n2 - 1)), 0));
    for (int r = r0; r <= R; ++r) {
        // the shell's square of columns, cut to the grid
        const int a0 = max(ci - r, 0), a1 = min(ci + r, n0 - 1), b0 = max(cj - r, 0), b1 = min(cj + r, n1 - 1);
        const int na = a1 - a0 + 1, nb = b1 - b0 + 1;
        if (na > 0 && nb > 0) {
            const int zl = ck - r, zh = ck + r;
            for (int it = sub; it < na * nb; it += LANES) {
                const int a = a0 + it / nb, b = b0 + it % nb;
                const int base = (a * n1 + b) * n2;
                if (a == ci - r || a == ci + r || b == cj - r || b == cj + r) {      // rim: the column's whole run
                    const int z0 = max(zl, 0), z1 = min(zh, n2 - 1);
                    if (z0 <= z1) best = run(start[base + z0], start[base + z1 + 1], best);
                } else {                                                             // inside: the two end cells
                    if (zl >= 0 && zl < n2) best = run(start[base + zl], start[base + zl + 1], best);
                    if (zh >= 0 && zh < n2) best = run(start[base + zh], start[base + zh + 1], best);
                }
            }
        }
        best = lanes_min<LANES>(best);
        const float rw = (float)r * w;
        if (best <= rw * rw) break;
        // every cell of the grid has been visited
        if (ci - r <= 0 && ci + r >= n0 - 1 && cj - r <= 0 && cj + r >= n1 - 1 && ck - r <= 0 && ck + r >= n2 - 1) break;
    }
    return best;
}

// One launch over the queries: d2[j] = the walk's minimum for query j.  Src is what the cells hold: Src::LANES lanes per query, and
// src.run(p, hi, x, y, z, best) -> best over payload slots [p, hi).
template <class Src>
__global__ __launch_bounds__(256) void shell_query_kernel(const float* __restrict__ q, const long long* __restrict__ n_dev,
                                                          long long n_host, Grid g, int R, float w, float cap2, const Src src,
                                                          const int* __restrict__ start, float* __restrict__ d2) {
    const long long Q = dev_count(n_dev, n_host);
    const int sub = threadIdx.x % Src::LANES;
    for (long long j = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / Src::LANES; j < Q;
         j += ((long long)gridDim.x * blockDim.x) / Src::LANES) {
        const float x = q[3 * j], y = q[3 * j + 1], z = q[3 * j + 2];
        const float best = shell_walk<Src::LANES>(g, R, w, cap2, start, sub, x, y, z,
                                                  [&](int p, int hi, float b) { return src.run(p, hi, x, y, z, b); });
        if (sub == 0) d2[j] = best;
    }
}

template <class Src>
int shell_query(const Src& src, const int* start, const Grid& g, float cap, float w, const float* q3, long long Q, const long long* Q_dev,
                float* d2, hipStream_t st) {
    if (Q == 0) return 0;
    const int R = (int)ceil((double)cap / (double)w);               // <= 2^24 (nn_cap_ok)
    shell_query_kernel<Src><<<nbp_ew_grid(Q * Src::LANES, 256), 256, 0, st>>>(q3, Q_dev, Q, g, R, w, cap * cap, src, start, d2);
    return nbp_launch_status();
}

// A run of sorted points [p, hi), UNROLL of them in flight together (one per iteration is a chain of dependent round trips):
// visit(t, d, best) -> best for each point t at fp32 squared distance d from (x, y, z).
template <int UNROLL, class Visit>
__device__ __forceinline__ float point_run(const float4* __restrict__ sorted, int p, int hi, float x, float y, float z, float best,
                                           Visit visit) {
    for (; p + UNROLL <= hi; p += UNROLL) {
        float4 t[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) t[u] = sorted[p + u];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const float ex = t[u].x - x, ey = t[u].y - y, ez = t[u].z - z;
            best = visit(t[u], (ex * ex + ey * ey) + ez * ez, best);
        }
    }
    for (; p < hi; ++p) {
        const float4 t = sorted[p];
        const float ex = t.x - x, ey = t.y - y, ez = t.z - z;
        best = visit(t, (ex * ex + ey * ey) + ez * ez, best);
    }
    return best;
}

}  // namespace
