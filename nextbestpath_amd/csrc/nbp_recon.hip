// nbp_recon.hip -- reconstruction-quality metrics: exact truncated nearest-neighbour distances between two point sets that are
// already on the device, and their reproducible summary (include/nbp_hip.h: nbp_nn_*, nbp_recon_stats_f64; the definition of
// record is nextbestpath_amd/utility/recon_metrics.py).  Not in the reference.
//
// Nearest neighbour.  The targets inside the caller's box are counting-sorted into a uniform grid (bin, grid_exclusive_scan,
// scatter to float4 -- the coverage plan's three steps).  One launch over the queries follows: nbp_shell_walk.h's walk over the
// shells of cells around the query's unclamped cell, NN_LANES lanes per query, a run of cells being a run of the sorted array.  Its
// header proves that the result is the brute-force minimum over all in-box targets, bit for bit; and -- a minimum being blind to
// the order of its operands -- the atomicAdd slot order inside a cell does not show: two runs give the same bits.
//
// Summary (nbp_recon_stats_f64): nbp_stat_rows.h's fixed-order fold over STATS_BLOCKS blocks, a row being two float64 sums and the
// threshold counts.  No floating-point atomics: two runs give the same bits.
//
// Per-step curve (nbp_recon_curve_update_batch_f32).  The cloud is append-only and the GT fixed, so both directions
// are incremental: a point's distance to the GT never changes (it is queried once, in the step that appends it), and the minimum
// over a union is the minimum of the minima (a running per-GT-point minimum d2_gt is lowered by the new points only).  One walk
// per new point serves both: its NN_LANES lanes visit EVERY GT cell within Chebyshev distance R of its unclamped cell (the shell
// walk's early exit does not apply: the scatter needs every target within reach), each (x, y) column one contiguous run.  The lanes
// keep the point's own minimum (its accuracy distance), and a visited GT point with d < d2_gt[g] is lowered by an INTEGER atomicMin on
// the bit pattern: non-negative finite floats order like their bits and a minimum is blind to arrival order, so d2_gt is exact and
// two runs give the same bits.  The plain read that filters the atomic may be stale (another XCD's L2): values only decrease, so
// a stale read costs a redundant atomic, never a missed one.  What the walk leaves out is farther than R w >= cap (the walk's
// argument with r = R).  The slot -> GT index map is the fourth component of the plan's float4 (its bits; the query never reads it).
// The summaries follow in two launches of the stats geometry above: d2_gt in full, the step's own distances into the running
// float64 totals by one thread.  The watermark `seen` moves in the last launch only (the first two read it).
#include "nbp_shell_walk.h"
#include "nbp_stat_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int NN_LANES = 8;                      // lanes per query: the 8 rim columns of shell 1 at once
constexpr int NN_UNROLL = 4;                     // points of a run in flight together (coverage_mark_body: one per iteration
                                                 // is a chain of dependent round trips)
constexpr int STATS_BLOCKS = 256, STATS_THREADS = STAT_THREADS;
constexpr int STATS_MAX_T = 8;
constexpr int STATS_SUMS = 2, STATS_ROW = STATS_SUMS + STATS_MAX_T;   // 8-byte words of a block's row: two float64 sums, then the counts

// ---- sort
__global__ __launch_bounds__(256) void nn_bin_kernel(const float* __restrict__ t, const long long* __restrict__ n_dev, long long n_host,
                                                     Grid g, Box bx, int* __restrict__ cell_of, int* __restrict__ slot_of,
                                                     int* __restrict__ count) {
    const long long n = dev_count(n_dev, n_host);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = t[3 * i], y = t[3 * i + 1], z = t[3 * i + 2];
        int c = -1;
        if (in_box(g, bx, x, y, z)) {
            c = grid_cell(g, x, y, z, nullptr);
            slot_of[i] = atomicAdd(&count[c], 1);
        }
        cell_of[i] = c;
    }
}

__global__ __launch_bounds__(256) void nn_scatter_kernel(const float* __restrict__ t, const long long* __restrict__ n_dev,
                                                         long long n_host, const int* __restrict__ cell_of,
                                                         const int* __restrict__ slot_of, const int* __restrict__ start,
                                                         float4* __restrict__ sorted) {
    const long long n = dev_count(n_dev, n_host);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = cell_of[i];
        if (c >= 0) sorted[start[c] + slot_of[i]] = make_float4(t[3 * i], t[3 * i + 1], t[3 * i + 2], __int_as_float((int)i));   // .w: the target's index (curve walk)
    }
}

// ---- query: the shell walk over cells of sorted points
struct NNPoints {
    static constexpr int LANES = NN_LANES;
    const float4* __restrict__ sorted;
    __device__ __forceinline__ float run(int p, int hi, float x, float y, float z, float best) const {
        return point_run<NN_UNROLL>(sorted, p, hi, x, y, z, best, [](const float4&, float d, float b) { return d < b ? d : b; });
    }
};

// ---- summary
struct StatsThresholds { float v[STATS_MAX_T]; };

// One block of the fixed geometry: row = the block's two float64 sums and its T counts (the words beyond them are not written, and
// nothing reads them: a fold takes the columns below 2 + T).  The counts are independent of one another and of the sums: a larger
// T moves no bit of the rest.
template <int T>
__device__ __forceinline__ void stats_block(const float* __restrict__ d2, long long n, const float* th, int block,
                                            unsigned long long* __restrict__ row) {
    double s[STATS_SUMS] = {0.0, 0.0};
    long long c[T];
#pragma unroll
    for (int t = 0; t < T; ++t) c[t] = 0;
    for (long long i = (long long)block * STATS_THREADS + threadIdx.x; i < n; i += (long long)STATS_BLOCKS * STATS_THREADS) {
        const float v = d2[i];
        s[0] += sqrt((double)v);
        s[1] += (double)v;
#pragma unroll
        for (int t = 0; t < T; ++t) c[t] += v <= th[t] ? 1 : 0;
    }
    stat_row_store<STATS_SUMS, T>(s, c, row);
}

// Column col of the STATS_BLOCKS rows, added in index order
__device__ __forceinline__ unsigned long long stats_fold(const unsigned long long* __restrict__ rows, int col) {
    return stat_rows_fold(rows, STATS_BLOCKS, STATS_ROW, STATS_SUMS, col);
}

template <int T>
__global__ __launch_bounds__(STATS_THREADS) void stats_partial_kernel(const float* __restrict__ d2, const long long* __restrict__ n_dev,
                                                                     long long n_host, StatsThresholds th,
                                                                     unsigned long long* __restrict__ rows) {
    stats_block<T>(d2, dev_count(n_dev, n_host), th.v, blockIdx.x, rows + (size_t)blockIdx.x * STATS_ROW);
}

__global__ __launch_bounds__(64) void stats_final_kernel(const unsigned long long* __restrict__ rows, int T, double* __restrict__ sums,
                                                         long long* __restrict__ counts) {
    const int col = threadIdx.x;
    if (col < 2) sums[col] = __longlong_as_double((long long)stats_fold(rows, col));
    else if (col < 2 + T) counts[col - 2] = (long long)stats_fold(rows, col);
}

template <int T>
void launch_stats(hipStream_t st, const float* d2, const long long* n_dev, long long n, const StatsThresholds& th,
                  unsigned long long* rows) {
    stats_partial_kernel<T><<<STATS_BLOCKS, STATS_THREADS, 0, st>>>(d2, n_dev, n, th, rows);
}

// ---- per-step curve
constexpr int CURVE_BATCH = 16;
constexpr int CURVE_TOTALS = 2 + STATS_MAX_T;    // 8-byte words of an item's running accuracy totals: two float64 sums, the counts

struct CurveItem {
    Grid g;
    Box bx;
    int R;
    float cap2;
    int T, G;
    unsigned gx_walk;
    const float4* sorted;
    const int* start;
    const float* cloud;
    long long capacity, n_gt;
    const long long* count;
    long long* seen;
    unsigned* d2_gt;
    float* d2_new;
    unsigned long long* totals;
    double* row;
    unsigned long long* part;                    // [2][STATS_BLOCKS][STATS_ROW]: d2_gt's rows, then the step's
    float th[STATS_MAX_T];
};
struct CurveBatch { CurveItem it[CURVE_BATCH]; };

// The item's new rows [s, e): both ends from the device, e = min(count, capacity); s >= e: nothing new.
__device__ __forceinline__ void curve_range(const CurveItem& a, long long* s, long long* e) {
    long long seen = *a.seen, end = *a.count;
    end = end < 0 ? 0 : (end > a.capacity ? a.capacity : end);
    seen = seen < 0 ? 0 : seen;
    *s = seen;
    *e = seen >= end ? seen : end;
}

__global__ __launch_bounds__(256) void curve_walk_kernel(const CurveBatch b) {
    const CurveItem& a = b.it[blockIdx.y];
    if (blockIdx.x >= a.gx_walk) return;
    long long s, e;
    curve_range(a, &s, &e);
    const int sub = threadIdx.x % NN_LANES;
    const int n0 = a.g.n[0], n1 = a.g.n[1], n2 = a.g.n[2], R = a.R;
    unsigned* __restrict__ d2_gt = a.d2_gt;
    for (long long j = s + ((long long)blockIdx.x * blockDim.x + threadIdx.x) / NN_LANES; j < e;
         j += ((long long)a.gx_walk * blockDim.x) / NN_LANES) {
        const float x = a.cloud[3 * j], y = a.cloud[3 * j + 1], z = a.cloud[3 * j + 2];
        // as a target the point counts inside the box only, as a query wherever its cell is within reach of the grid (a far or NaN
        // point: cap2, no access)
        const bool scatter = in_box(a.g, a.bx, x, y, z);
        float best = a.cap2;
        int c[3];
        if (cell_in_reach(a.g, R, x, y, z, c)) {                   // (uniform over the point's lanes)
            const int a0 = max(c[0] - R, 0), a1 = min(c[0] + R, n0 - 1), b0 = max(c[1] - R, 0), b1 = min(c[1] + R, n1 - 1);
            const int z0 = max(c[2] - R, 0), z1 = min(c[2] + R, n2 - 1);
            const int na = a1 - a0 + 1, nb = b1 - b0 + 1;
            if (na > 0 && nb > 0 && z0 <= z1) {
                for (int it = sub; it < na * nb; it += NN_LANES) {
                    const int base = ((a0 + it / nb) * n1 + (b0 + it % nb)) * n2;
                    best = point_run<NN_UNROLL>(a.sorted, a.start[base + z0], a.start[base + z1 + 1], x, y, z, best,
                                                [=](const float4& t, float d, float m) {
                                                    if (scatter) {
                                                        const int gi = __float_as_int(t.w);
                                                        if (d < __uint_as_float(d2_gt[gi])) atomicMin(&d2_gt[gi], __float_as_uint(d));
                                                    }
                                                    return d < m ? d : m;
                                                });
                }
            }
            best = lanes_min<NN_LANES>(best);
        }
        if (sub == 0) a.d2_new[j - s] = best;
    }
}

// grid (STATS_BLOCKS, 2, n): y = 0 the whole of d2_gt, y = 1 the step's own distances
__global__ __launch_bounds__(STATS_THREADS) void curve_partial_kernel(const CurveBatch b) {
    const CurveItem& a = b.it[blockIdx.z];
    const int half = blockIdx.y;
    const float* d2 = (const float*)a.d2_gt;
    long long n = a.n_gt;
    if (half) {
        long long s, e;
        curve_range(a, &s, &e);
        d2 = a.d2_new;
        n = e - s;
    }
    stats_block<STATS_MAX_T>(d2, n, a.th, blockIdx.x, a.part + ((size_t)half * STATS_BLOCKS + blockIdx.x) * STATS_ROW);
}

// One block per item: the rows of either half added in index order (stats_fold), the step's sums added to the running totals by
// one thread, the item's row written, the watermark moved.
__global__ __launch_bounds__(64) void curve_final_kernel(const CurveBatch b) {
    const CurveItem& a = b.it[blockIdx.x];
    __shared__ unsigned long long tot[2][STATS_ROW];
    const int half = threadIdx.x / 32, col = threadIdx.x % 32;
    if (col < STATS_ROW) tot[half][col] = stats_fold(a.part + (size_t)half * STATS_BLOCKS * STATS_ROW, col);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s, e;
        curve_range(a, &s, &e);
        const int T = a.T;
        if (e > s) {                                               // (nothing new: the totals and the watermark stay)
            for (int c = 0; c < 2; ++c)
                a.totals[c] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a.totals[c]) +
                                                                       __longlong_as_double((long long)tot[1][c]));
            for (int t = 0; t < T; ++t) a.totals[2 + t] += tot[1][2 + t];
            *a.seen = e;
        }
        double* row = a.row;
        row[0] = __longlong_as_double((long long)a.totals[0]);
        row[1] = __longlong_as_double((long long)a.totals[1]);
        row[2] = __longlong_as_double((long long)tot[0][0]);
        row[3] = __longlong_as_double((long long)tot[0][1]);
        row[4] = (double)e;
        row[5] = (double)a.n_gt;
        for (int t = 0; t < T; ++t) {
            row[6 + t] = (double)(long long)a.totals[2 + t];
            row[6 + T + t] = (double)(long long)tot[0][2 + t];
        }
    }
}

// ---- host (the grid over the caller's box, the argument checks and the carves: nbp_nn_grid.h)
// a plan holds n = max(T, 1) sorted points; its build's scratch ends with their cell and slot
size_t nn_points(long long T) { return (size_t)(T > 0 ? T : 1); }
struct NNBuildWs { NNScratch s; int* cell_of; int* slot_of; };
NNBuildWs nn_build_ws_layout(Carver& c, size_t ncell, size_t n) { return {nn_scratch_layout(c, ncell), c.take<int>(n), c.take<int>(n)}; }
// nbp_nn_dist2_f32's workspace: the plan, then its build's scratch
constexpr size_t NN_DIST2_SLACK = 256;          // (historical: the scratch once aligned its own base behind the plan)
struct NNDist2Ws { NNPlan plan; NNBuildWs ws; };
NNDist2Ws nn_dist2_layout(Carver& c, size_t ncell, size_t n) { return {nn_plan_layout(c, ncell, n), nn_build_ws_layout(c, ncell, n)}; }
size_t nn_plan_bytes(size_t ncell, long long T) { return carved_bytes(0, nn_plan_layout, ncell, nn_points(T)); }
size_t nn_plan_ws_bytes(size_t ncell, long long T) { return carved_bytes(0, nn_build_ws_layout, ncell, nn_points(T)); }
size_t nn_dist2_ws_bytes(size_t ncell, long long T) { return carved_bytes(NN_DIST2_SLACK, nn_dist2_layout, ncell, nn_points(T)); }

int nn_build(const float* t3, long long T, const long long* T_dev, const BoxGrid& b, const NNPlan& pl, const NNBuildWs& w, hipStream_t st) {
    hipError_t e = hipMemsetAsync(w.s.count, 0, b.ncell * 4, st);
    if (e != hipSuccess) return (int)e;
    int rc;
    const int grid = nbp_ew_grid(T > 0 ? T : 1, 256);
    if (T > 0) {
        nn_bin_kernel<<<grid, 256, 0, st>>>(t3, T_dev, T, b.g, b.bx, w.cell_of, w.slot_of, w.s.count);
        if ((rc = nbp_launch_status())) return rc;
    }
    if ((rc = grid_exclusive_scan(w.s.count, (long long)b.ncell, w.s.tsum, pl.start, st))) return rc;
    if (T > 0) {
        nn_scatter_kernel<<<grid, 256, 0, st>>>(t3, T_dev, T, w.cell_of, w.slot_of, pl.start, pl.payload);
        if ((rc = nbp_launch_status())) return rc;
    }
    return 0;
}

int nn_query(const NNPlan& pl, const BoxGrid& b, float cap, float w, const float* q3, long long Q, const long long* Q_dev, float* d2,
             hipStream_t st) {
    return shell_query(NNPoints{pl.payload}, pl.start, b.g, cap, w, q3, Q, Q_dev, d2, st);
}

// a *_bytes function's grid: false is its refusal (0 bytes)
bool nn_bytes_grid(const float* lo, const float* hi, float cell, long long T, BoxGrid* b) {
    return nn_count_ok(T) && !nn_grid(lo, hi, cell, b);
}

}  // namespace

extern "C" size_t nbp_nn_plan_bytes(const float* lo_host, const float* hi_host, float cell, long long T) {
    BoxGrid b;
    return nn_bytes_grid(lo_host, hi_host, cell, T, &b) ? nn_plan_bytes(b.ncell, T) : 0;
}

extern "C" size_t nbp_nn_plan_workspace_bytes(const float* lo_host, const float* hi_host, float cell, long long T) {
    BoxGrid b;
    return nn_bytes_grid(lo_host, hi_host, cell, T, &b) ? nn_plan_ws_bytes(b.ncell, T) : 0;
}

extern "C" int nbp_nn_plan_build_f32(const float* t3, long long T, const long long* T_dev_or_null, const float* lo_host,
                                     const float* hi_host, float cell, void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                                     void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!plan || !ws || !nn_count_ok(T) || (T > 0 && !t3), NBP_E_ARG);
    BoxGrid b;
    const int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    NBP_RETURN_IF(plan_bytes < nn_plan_bytes(b.ncell, T) || ws_bytes < nn_plan_ws_bytes(b.ncell, T), NBP_E_WS);
    return nn_build(t3, T, T_dev_or_null, b, nn_plan_of(plan, b.ncell), carve(ws, nn_build_ws_layout, b.ncell, nn_points(T)), (hipStream_t)stream);
}

extern "C" int nbp_nn_dist2_planned_f32(const void* plan, const float* lo_host, const float* hi_host, float cell, float cap,
                                        const float* q3, long long Q, const long long* Q_dev_or_null, float* d2, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!plan || !nn_args_ok(lo_host, hi_host, cell) || !nn_cap_ok(cap, cell) || !nn_count_ok(Q), NBP_E_ARG);
    NBP_RETURN_IF(Q > 0 && (!q3 || !d2), NBP_E_ARG);
    BoxGrid b;
    const int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    return nn_query(nn_plan_of(plan, b.ncell), b, cap, cell, q3, Q, Q_dev_or_null, d2, (hipStream_t)stream);
}

extern "C" size_t nbp_nn_dist2_workspace_bytes(const float* lo_host, const float* hi_host, float cell, long long T) {
    BoxGrid b;
    return nn_bytes_grid(lo_host, hi_host, cell, T, &b) ? nn_dist2_ws_bytes(b.ncell, T) : 0;
}

extern "C" int nbp_nn_dist2_f32(const float* q3, long long Q, const long long* Q_dev_or_null, const float* t3, long long T,
                                const long long* T_dev_or_null, const float* lo_host, const float* hi_host, float cap, float cell,
                                float* d2, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!ws || !nn_args_ok(lo_host, hi_host, cell) || !nn_cap_ok(cap, cell), NBP_E_ARG);
    NBP_RETURN_IF(!nn_count_ok(Q) || !nn_count_ok(T) || (T > 0 && !t3) || (Q > 0 && (!q3 || !d2)), NBP_E_ARG);
    BoxGrid b;
    int rc = nn_grid(lo_host, hi_host, cell, &b);
    if (rc) return rc;
    NBP_RETURN_IF(ws_bytes < nn_dist2_ws_bytes(b.ncell, T), NBP_E_WS);
    const NNDist2Ws L = carve(ws, nn_dist2_layout, b.ncell, nn_points(T));
    if ((rc = nn_build(t3, T, T_dev_or_null, b, L.plan, L.ws, (hipStream_t)stream))) return rc;
    return nn_query(L.plan, b, cap, cell, q3, Q, Q_dev_or_null, d2, (hipStream_t)stream);
}

extern "C" size_t nbp_recon_stats_workspace_bytes(void) { return stat_rows_bytes(STATS_BLOCKS, STATS_ROW); }

extern "C" int nbp_recon_stats_f64(const float* d2, long long n, const long long* n_dev_or_null, int T, const float* thresholds_host,
                                   double* sums2, long long* counts, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!thresholds_host || !sums2 || !counts || !ws || n < 0 || (n > 0 && !d2) || T < 1 || T > STATS_MAX_T, NBP_E_ARG);
    for (int t = 0; t < T; ++t) NBP_RETURN_IF(!(thresholds_host[t] > 0) || !isfinite(thresholds_host[t]), NBP_E_ARG);
    NBP_RETURN_IF((((uintptr_t)sums2 | (uintptr_t)counts) & 7), NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < nbp_recon_stats_workspace_bytes(), NBP_E_WS);
    hipStream_t st = (hipStream_t)stream;
    StatsThresholds th;
    for (int t = 0; t < STATS_MAX_T; ++t) th.v[t] = sq_below(thresholds_host[t < T ? t : 0]);
    unsigned long long* rows = carve(ws, stat_rows_layout, (size_t)STATS_BLOCKS, STATS_ROW);
    switch (T) {
        case 1: launch_stats<1>(st, d2, n_dev_or_null, n, th, rows); break;
        case 2: launch_stats<2>(st, d2, n_dev_or_null, n, th, rows); break;
        case 3: launch_stats<3>(st, d2, n_dev_or_null, n, th, rows); break;
        case 4: launch_stats<4>(st, d2, n_dev_or_null, n, th, rows); break;
        case 5: launch_stats<5>(st, d2, n_dev_or_null, n, th, rows); break;
        case 6: launch_stats<6>(st, d2, n_dev_or_null, n, th, rows); break;
        case 7: launch_stats<7>(st, d2, n_dev_or_null, n, th, rows); break;
        default: launch_stats<8>(st, d2, n_dev_or_null, n, th, rows); break;
    }
    const int rc = nbp_launch_status();
    if (rc) return rc;
    stats_final_kernel<<<1, 64, 0, st>>>(rows, T, sums2, counts);
    return nbp_launch_status();
}

extern "C" size_t nbp_recon_curve_workspace_bytes(int n) {
    if (n < 1 || n > CURVE_BATCH) return 0;
    return stat_rows_bytes((size_t)n * 2 * STATS_BLOCKS, STATS_ROW);
}

extern "C" size_t nbp_recon_curve_totals_bytes(void) { return (size_t)CURVE_TOTALS * 8; }

extern "C" int nbp_recon_curve_update_batch_f32(int n, const void* const* plans, const int* G, const float* lo_host,
                                                const float* hi_host, const float* cell, const float* cap, const float* const* cloud3,
                                                const long long* capacity, const long long* const* count_dev, long long* const* seen_dev,
                                                float* const* d2_gt, float* const* d2_new, void* const* totals, const int* T,
                                                const float* thresholds_host, double* const* row, const long long* new_bound, void* ws,
                                                size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(n < 1 || n > CURVE_BATCH || !plans || !G || !lo_host || !hi_host || !cell || !cap || !cloud3 || !capacity ||
                  !count_dev || !seen_dev || !d2_gt || !d2_new || !totals || !T || !thresholds_host || !row || !new_bound || !ws,
                  NBP_E_ARG);
    NBP_RETURN_IF(ws_bytes < nbp_recon_curve_workspace_bytes(n), NBP_E_WS);
    unsigned long long* part = carve(ws, stat_rows_layout, (size_t)n * 2 * STATS_BLOCKS, STATS_ROW);
    CurveBatch b;
    unsigned gwalk = 1;
    for (int r = 0; r < CURVE_BATCH; ++r) {
        const int q = r < n ? r : 0;
        const float* lo = lo_host + 3 * q;
        const float* hi = hi_host + 3 * q;
        NBP_RETURN_IF(!plans[q] || !cloud3[q] || !count_dev[q] || !seen_dev[q] || !d2_gt[q] || !d2_new[q] || !totals[q] || !row[q] ||
                      G[q] < 1 || capacity[q] < 1 || capacity[q] > 0x7fffffffll || new_bound[q] < 0 || T[q] < 1 || T[q] > STATS_MAX_T ||
                      !nn_args_ok(lo, hi, cell[q]) || !nn_cap_ok(cap[q], cell[q]),
                      NBP_E_ARG);
        NBP_RETURN_IF((((uintptr_t)totals[q] | (uintptr_t)row[q] | (uintptr_t)seen_dev[q] | (uintptr_t)count_dev[q]) & 7), NBP_E_SHAPE);
        CurveItem& a = b.it[r];
        BoxGrid bg;
        const int rc = nn_grid(lo, hi, cell[q], &bg);
        if (rc) return rc;
        a.g = bg.g; a.bx = bg.bx;
        const NNPlan pl = nn_plan_of(plans[q], bg.ncell);
        a.sorted = pl.payload; a.start = pl.start;
        a.R = (int)ceil((double)cap[q] / (double)cell[q]);
        a.cap2 = cap[q] * cap[q];
        a.T = T[q]; a.G = G[q]; a.n_gt = G[q];
        for (int t = 0; t < STATS_MAX_T; ++t) {
            const float thr = thresholds_host[STATS_MAX_T * q + (t < T[q] ? t : 0)];
            NBP_RETURN_IF(!(thr > 0) || !isfinite(thr), NBP_E_ARG);
            a.th[t] = sq_below(thr);
        }
        a.cloud = cloud3[q]; a.capacity = capacity[q]; a.count = count_dev[q]; a.seen = seen_dev[q];
        a.d2_gt = (unsigned*)d2_gt[q]; a.d2_new = d2_new[q]; a.totals = (unsigned long long*)totals[q]; a.row = row[q];
        a.part = part + (size_t)q * 2 * STATS_BLOCKS * STATS_ROW;
        const long long work = new_bound[q] < capacity[q] ? new_bound[q] : capacity[q];
        a.gx_walk = r < n ? (unsigned)nbp_ew_grid((work > 0 ? work : 1) * NN_LANES, 256) : 0;
        if (a.gx_walk > gwalk) gwalk = a.gx_walk;
    }
    hipStream_t st = (hipStream_t)stream;
    curve_walk_kernel<<<dim3(gwalk, (unsigned)n), 256, 0, st>>>(b);
    int rc = nbp_launch_status();
    if (rc) return rc;
    curve_partial_kernel<<<dim3(STATS_BLOCKS, 2, (unsigned)n), STATS_THREADS, 0, st>>>(b);
    if ((rc = nbp_launch_status())) return rc;
    curve_final_kernel<<<(unsigned)n, 64, 0, st>>>(b);
    return nbp_launch_status();
}
