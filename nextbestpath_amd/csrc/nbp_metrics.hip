// nbp_metrics.hip -- planner-facing validation metrics of one batch, per sample, on the device (include/nbp_hip.h:
// nbp_val_metrics_f32; the definition of record is nextbestpath_amd/utility/metrics.py).
//
// Obstacle pass (obst_kernel<T>): out2 and gt are read once, 16 bytes per lane.  Every comparison `out2 >= tau[t]` and `gt > 0.5`
// of a wave is a 64-bit lane mask (a ballot); the counts are popcounts of those masks and of their ANDs, kept in wave-uniform
// integers: nothing is reduced across lanes.  Per wave: the label count and, per threshold, the predicted and the true-positive
// counts; the four waves of a workgroup meet in LDS, and the workgroup adds (tp, fp, fn, tn) to the sample's slots with one
// 64-bit integer atomic each (the slots are zeroed by a memset in front of the launch on the same stream).  Integer sums only:
// exact and independent of the order of arrival.
//
// Ranking pass (rank_kernel): one workgroup per sample.  It scans the unsorted `bidx` in chunks of one entry per thread and compacts
// the sample's good targets IN RECORD ORDER (ballot + popcount of the lower lanes inside a wave, the waves' counts through LDS); a
// target's range test comes before the gather from out1, so a bad coordinate is never turned into an address.  Up to RANK_CAP
// pairs (p, g) are held in LDS and the pairs i < j are strided over from there (lane l reads entry j = i_l + 1 + s: consecutive
// addresses).  A sample with more good targets than RANK_CAP takes the same loops over the RAW entries instead (membership, range
// test and gather repeated per visit: slow, correct, never met by real records, which hold a few dozen targets).
// Sums: integers, and two float64 sums that every thread accumulates over its own entries in index order and that are then added
// by a fixed tree (shuffles inside a wave, the four waves in order): two runs give the same bits.  No floating-point atomics.
#include "common.h"

#include <stddef.h>

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_WAVES = MET_THREADS / 64;
constexpr int MET_MAX_T = 8;
constexpr int OBST_QUADS = 4;                    // 16-byte loads per thread and input before a workgroup's grid stride
constexpr int RANK_CAP = 2048;                   // (p, g) pairs held in LDS: 16 KiB

struct Thresholds {
    float v[MET_MAX_T];
};

template <int T>
__global__ __launch_bounds__(MET_THREADS) void obst_kernel(const float4* __restrict__ out2, const float4* __restrict__ gt,
                                                            int quads_per_sample, Thresholds th,
                                                            unsigned long long* __restrict__ obst) {
    __shared__ int part[MET_WAVES][2 * MET_MAX_T + 2];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const float4* __restrict__ o = out2 + (size_t)b * quads_per_sample;
    const float4* __restrict__ l = gt + (size_t)b * quads_per_sample;
    int n_px = 0, n_label = 0, n_pred[T], n_tp[T];               // wave-uniform
#pragma unroll
    for (int t = 0; t < T; ++t) n_pred[t] = n_tp[t] = 0;
    for (int q = blockIdx.x * MET_THREADS + tid; q < quads_per_sample; q += gridDim.x * MET_THREADS) {
        const float4 v = o[q];
        const float4 w = l[q];
        const float ve[4] = {v.x, v.y, v.z, v.w};
        const float we[4] = {w.x, w.y, w.z, w.w};
        n_px += 4 * __popcll(__ballot(1));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned long long lab = __ballot(we[e] > 0.5f);
            n_label += __popcll(lab);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const unsigned long long pred = __ballot(ve[e] >= th.v[t]);      // a NaN compares false: negative
                n_pred[t] += __popcll(pred);
                n_tp[t] += __popcll(pred & lab);
            }
        }
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        part[wave][0] = n_px;
        part[wave][1] = n_label;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            part[wave][2 + 2 * t] = n_pred[t];
            part[wave][3 + 2 * t] = n_tp[t];
        }
    }
    __syncthreads();
    if (tid < T) {
        long long px = 0, lab = 0, pred = 0, tp = 0;
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) {
            px += part[w][0];
            lab += part[w][1];
            pred += part[w][2 + 2 * tid];
            tp += part[w][3 + 2 * tid];
        }
        if (px > 0) {
            const long long fp = pred - tp, fn = lab - tp;
            unsigned long long* slot = obst + ((size_t)b * T + tid) * 4;
            atomicAdd(slot + 0, (unsigned long long)tp);
            atomicAdd(slot + 1, (unsigned long long)fp);
            atomicAdd(slot + 2, (unsigned long long)fn);
            atomicAdd(slot + 3, (unsigned long long)(px - tp - fp - fn));
        }
    }
}

// ---- ranking pass
struct Target {
    bool good;                                   // a member of the sample whose coordinates are inside the value map
    bool bad;                                    // a member whose coordinates are not
    float p, g;
};

// Entry k of the raw lists as seen by sample b.  The range test precedes the gather.
__device__ __forceinline__ Target load_target(const float* __restrict__ out1, const long long* __restrict__ coords,
                                              const float* __restrict__ gains, const long long* __restrict__ bidx, int k, int b,
                                              int V) {
    Target t = {false, false, 0.f, 0.f};
    if (bidx[k] != (long long)b) return t;
    const long long c = coords[3 * (size_t)k], row = coords[3 * (size_t)k + 1], col = coords[3 * (size_t)k + 2];
    if (c < 0 || c >= 8 || row < 0 || row >= V || col < 0 || col >= V) {
        t.bad = true;
        return t;
    }
    t.good = true;
    t.p = out1[(((size_t)b * 8 + (size_t)c) * V + (size_t)row) * V + (size_t)col];
    t.g = gains[k];
    return t;
}

struct Best {                                    // the candidate for pred_best: idx < 0 = none yet
    int idx;
    float p, g;
};

// a NaN never beats a number; the larger p wins; equal p (or two NaNs): the earlier target
__device__ __forceinline__ Best better(const Best a, const Best b) {
    if (a.idx < 0) return b;
    if (b.idx < 0) return a;
    const bool na = a.p != a.p, nb = b.p != b.p;
    if (na != nb) return na ? b : a;
    if (!na && a.p != b.p) return a.p > b.p ? a : b;
    return a.idx < b.idx ? a : b;
}

struct Acc {
    unsigned long long comparable, concordant, discordant;
    double sum_abs, sum_sq;
    float gmax;
    Best best;
};

__device__ __forceinline__ void acc_pair(Acc& a, float pi, float gi, float pj, float gj) {
    if (gi != gj) {
        a.comparable += 1;
        const bool up = gi > gj, down = gi < gj;
        a.concordant += ((pi > pj) && up) || ((pi < pj) && down);
        a.discordant += ((pi > pj) && down) || ((pi < pj) && up);
    }
}

__device__ __forceinline__ void acc_single(Acc& a, int idx, float p, float g) {
    const double d = (double)p - (double)g;
    a.sum_abs += fabs(d);
    a.sum_sq += d * d;
    a.gmax = g > a.gmax ? g : a.gmax;
    a.best = better(a.best, Best{idx, p, g});
}

__global__ __launch_bounds__(MET_THREADS) void rank_kernel(const float* __restrict__ out1, const long long* __restrict__ coords,
                                                            const float* __restrict__ gains, const long long* __restrict__ bidx,
                                                            int V, int K, long long* __restrict__ rank, double* __restrict__ val) {
    __shared__ float sp[RANK_CAP], sg[RANK_CAP];
    __shared__ int wave_good[MET_WAVES], wave_bad[MET_WAVES];
    __shared__ Acc wave_acc[MET_WAVES];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. the sample's good targets, compacted in record order
    int n = 0, n_bad = 0;                                           // block-uniform
    for (int k0 = 0; k0 < K; k0 += MET_THREADS) {
        const int k = k0 + tid;
        Target t = {false, false, 0.f, 0.f};
        if (k < K) t = load_target(out1, coords, gains, bidx, k, b, V);
        const unsigned long long mg = __ballot(t.good), mb = __ballot(t.bad);
        if (lane == 0) {
            wave_good[wave] = __popcll(mg);
            wave_bad[wave] = __popcll(mb);
        }
        __syncthreads();
        int pos = n + __popcll(mg & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) {
            if (w < wave) pos += wave_good[w];
            n += wave_good[w];
            n_bad += wave_bad[w];
        }
        if (t.good && pos < RANK_CAP) {
            sp[pos] = t.p;
            sg[pos] = t.g;
        }
        __syncthreads();
    }

    // 2. every thread: its entries i (strided), and for each the pairs (i, j > i)
    Acc a = {0ull, 0ull, 0ull, 0.0, 0.0, -INFINITY, Best{-1, 0.f, 0.f}};
    if (n <= RANK_CAP) {
        for (int i = tid; i < n; i += MET_THREADS) {
            const float pi = sp[i], gi = sg[i];
            acc_single(a, i, pi, gi);
            for (int j = i + 1; j < n; ++j) acc_pair(a, pi, gi, sp[j], sg[j]);
        }
    } else {
        for (int i = tid; i < K; i += MET_THREADS) {
            const Target ti = load_target(out1, coords, gains, bidx, i, b, V);
            if (!ti.good) continue;
            acc_single(a, i, ti.p, ti.g);
            for (int j = i + 1; j < K; ++j) {
                const Target tj = load_target(out1, coords, gains, bidx, j, b, V);
                if (tj.good) acc_pair(a, ti.p, ti.g, tj.p, tj.g);
            }
        }
    }

    // 3. a fixed tree: shuffles inside the wave, then the waves in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.comparable += __shfl_down(a.comparable, off, 64);
        a.concordant += __shfl_down(a.concordant, off, 64);
        a.discordant += __shfl_down(a.discordant, off, 64);
        a.sum_abs += __shfl_down(a.sum_abs, off, 64);
        a.sum_sq += __shfl_down(a.sum_sq, off, 64);
        const float og = __shfl_down(a.gmax, off, 64);
        a.gmax = og > a.gmax ? og : a.gmax;
        Best o;
        o.idx = __shfl_down(a.best.idx, off, 64);
        o.p = __shfl_down(a.best.p, off, 64);
        o.g = __shfl_down(a.best.g, off, 64);
        a.best = better(a.best, o);
    }
    if (lane == 0) wave_acc[wave] = a;
    __syncthreads();
    if (tid == 0) {
        Acc r = wave_acc[0];
#pragma unroll
        for (int w = 1; w < MET_WAVES; ++w) {
            const Acc o = wave_acc[w];
            r.comparable += o.comparable;
            r.concordant += o.concordant;
            r.discordant += o.discordant;
            r.sum_abs += o.sum_abs;
            r.sum_sq += o.sum_sq;
            r.gmax = o.gmax > r.gmax ? o.gmax : r.gmax;
            r.best = better(r.best, o.best);
        }
        long long* rk = rank + (size_t)b * 6;
        double* vl = val + (size_t)b * 4;
        rk[0] = n;
        rk[1] = n_bad;
        rk[2] = (long long)r.comparable;
        rk[3] = (long long)r.concordant;
        rk[4] = (long long)r.discordant;
        rk[5] = (n > 0 && r.best.g == r.gmax) ? 1 : 0;
        vl[0] = n > 0 ? r.sum_abs : 0.0;
        vl[1] = n > 0 ? r.sum_sq : 0.0;
        vl[2] = n > 0 ? (double)r.gmax : 0.0;
        vl[3] = n > 0 ? (double)r.best.g : 0.0;
    }
}

template <int T>
void launch_obst(dim3 grid, hipStream_t st, const float* out2, const float* gt, int quads, const Thresholds& th, long long* obst) {
    obst_kernel<T><<<grid, MET_THREADS, 0, st>>>((const float4*)out2, (const float4*)gt, quads, th, (unsigned long long*)obst);
}

}  // namespace

extern "C" int nbp_val_metrics_f32(const float* out1, const float* out2, const float* gt, const long long* coords,
                                   const float* gains, const long long* bidx, int B, int S, int K, int T,
                                   const float* thresholds_host, long long* obst, long long* rank, double* val, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!out1 || !out2 || !gt || !thresholds_host || !obst || !rank || !val, NBP_E_ARG);
    NBP_RETURN_IF(B < 1 || K < 0 || T < 1 || T > MET_MAX_T, NBP_E_ARG);
    NBP_RETURN_IF(K > 0 && (!coords || !gains || !bidx), NBP_E_ARG);
    NBP_RETURN_IF(S < 4 || S % 4 || S > 16384 || B > 65535, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)out2 | (uintptr_t)gt) & 15) || (((uintptr_t)obst | (uintptr_t)rank | (uintptr_t)val) & 7), NBP_E_SHAPE);
    hipStream_t st = (hipStream_t)stream;
    Thresholds th;
    for (int t = 0; t < MET_MAX_T; ++t) th.v[t] = thresholds_host[t < T ? t : 0];
    const int quads = S * S / 4;                                    // S % 4 == 0: a sample is a whole number of 16-byte quads
    hipError_t e = hipMemsetAsync(obst, 0, (size_t)B * T * 4 * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    int bx = (int)nbp_cdiv(quads, MET_THREADS * OBST_QUADS);
    if (bx > 64) bx = 64;
    const dim3 grid((unsigned)bx, (unsigned)B);
    switch (T) {
        case 1: launch_obst<1>(grid, st, out2, gt, quads, th, obst); break;
        case 2: launch_obst<2>(grid, st, out2, gt, quads, th, obst); break;
        case 3: launch_obst<3>(grid, st, out2, gt, quads, th, obst); break;
        case 4: launch_obst<4>(grid, st, out2, gt, quads, th, obst); break;
        case 5: launch_obst<5>(grid, st, out2, gt, quads, th, obst); break;
        case 6: launch_obst<6>(grid, st, out2, gt, quads, th, obst); break;
        case 7: launch_obst<7>(grid, st, out2, gt, quads, th, obst); break;
        default: launch_obst<8>(grid, st, out2, gt, quads, th, obst); break;
    }
    rank_kernel<<<dim3((unsigned)B), MET_THREADS, 0, st>>>(out1, coords, gains, bidx, S / 4, K, rank, val);
    return nbp_launch_status();
}
