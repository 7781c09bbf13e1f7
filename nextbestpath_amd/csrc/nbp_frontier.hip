// nbp_frontier.hip -- frontier-based exploration as a policy behind the network's interface (include/nbp_hip.h:
// nbp_frontier_workspace_bytes, nbp_frontier_mask_u64, nbp_frontier_policy_f32; the definition, which this file equals bit for bit,
// is nextbestpath_amd/utility/frontier.py).
//
// maps6 [B,6,S,S] -> the planner's two inputs, out1 [B,8,V,V] (frontier pixels in each value cell's eight disc sectors) and
// out2 [B,1,S,S] (unknown space as obstacle, or zero).  Everything after the first read works on bit-packed rows of W = S / 64
// 64-bit words (bit i of word w = column 64 w + i).  Five launches in stream order, no atomics, no hand-off between workgroups:
//   pack      a wave reads 64 consecutive pixels of the six planes; two ballots are the `seen` and `occupied` words
//   dilate    a thread owns one word of `near_d`: ORs of neighbouring rows, shifts with carries across the word seam
//   erode     a thread owns one word of `unknown`: the other half of the closing (ANDs; pixels outside the domain count as set)
//   frontier  a wave owns one word: free & (the unknown words of the four neighbours, shifted); lane i writes pixel i of out2
//   gain      a workgroup owns 64 value cells of one value row of one map: the 1 + 2 R pixel rows of its 6 frontier words in LDS
//             (3 KB) beside the [8][2 R + 1] sector masks (4 KB, expanded from the per-row column intervals the host passes as
//             kernel arguments); four neighbouring lanes share a cell, each takes every fourth row: one funnel shift across two
//             words and, where the window is not empty, eight popcounts; two shuffles add the four partial counts
// The call reads 24 S^2 bytes per map and writes 5.5 S^2.  It is not yet at the bound that reading its input sets: measured at
// four to five times a device copy of the same bytes, because five short launches depend on one another.
#include "nbp_internal.h"
#include <mutex>

namespace {

typedef unsigned long long u64;

constexpr int FR_THREADS = 256;
constexpr int FR_WAVES = FR_THREADS / 64;
constexpr int FR_MAX_R = NBP_FR_MAX_R, FR_MAX_D = NBP_FR_MAX_D;
constexpr int FR_ROWS = NBP_FR_ROWS;               // rows (and bits) of a sector mask
constexpr int FR_VC = 64, FR_PARTS = 4;            // value cells of a gain workgroup (one value row), lanes per cell
constexpr int FR_GAIN_THREADS = FR_VC * FR_PARTS;
constexpr int FR_LROWS = 2 * FR_MAX_R + 1;                        // 63 pixel rows ...
constexpr int FR_LWORDS = 4 * FR_VC / 64 + 2;                     // ... of 4 words and one more on either side
constexpr int FR_MAX_GRID = 1 << 20;

typedef NbpSectorRows SectorRows;                  // (nbp_internal.h: one column interval per heading and row)

// ---- pack: word g (of B S W, row-major over map, row, word) <- ballots over its 64 pixels
__global__ __launch_bounds__(FR_THREADS) void frontier_pack_kernel(const float* __restrict__ maps6, long long n_words, int S, int W,
                                                                   u64* __restrict__ seen, u64* __restrict__ occ) {
    const int lane = threadIdx.x & 63;
    const size_t plane = (size_t)S * S;
    const long long per_map = (long long)S * W;
    for (long long g = (long long)blockIdx.x * FR_WAVES + (threadIdx.x >> 6); g < n_words; g += (long long)gridDim.x * FR_WAVES) {
        const long long b = g / per_map, in_map = g - b * per_map;             // in_map = row W + word
        const int row = (int)(in_map / W), w = (int)(in_map - (long long)row * W);
        const float* p = maps6 + (size_t)b * 6 * plane + (size_t)in_map * 64 + lane;
        const float m0 = p[0], m1 = p[plane], m2 = p[2 * plane], m3 = p[3 * plane], m4 = p[4 * plane], m5 = p[5 * plane];
        const bool dom = row >= 1 && (w > 0 || lane >= 1);
        const u64 s = __ballot(dom && (m0 > 0.f || m1 > 0.f || m2 > 0.f || m3 > 0.f || m4 > 0.f));
        const u64 o = __ballot(dom && m5 > 0.f);
        if (lane == 0) { seen[g] = s; occ[g] = o; }
    }
}

// `seen` dilated by d (Chebyshev) at word (row, w) of one map
__device__ __forceinline__ u64 dilated_word(const u64* __restrict__ seen, int S, int W, int row, int w, int d) {
    u64 l = 0, c = 0, r = 0;
    const int r0 = row - d < 0 ? 0 : row - d, r1 = row + d > S - 1 ? S - 1 : row + d;
    for (int q = r0; q <= r1; ++q) {
        const u64* line = seen + (size_t)q * W;
        c |= line[w];
        if (w > 0) l |= line[w - 1];
        if (w + 1 < W) r |= line[w + 1];
    }
    u64 out = c;
    for (int k = 1; k <= d; ++k)           // 64 - k is 56..63: no shift by 64
        out |= (c << k) | (l >> (64 - k)) | (c >> k) | (r << (64 - k));
    return out;
}

// ---- dilate: word g of near_d
__global__ __launch_bounds__(FR_THREADS) void frontier_dilate_kernel(const u64* __restrict__ seen, long long n_words, int S, int W, int d,
                                                                     u64* __restrict__ near_d) {
    const long long per_map = (long long)S * W;
    for (long long g = (long long)blockIdx.x * FR_THREADS + threadIdx.x; g < n_words; g += (long long)gridDim.x * FR_THREADS) {
        const long long b = g / per_map, in_map = g - b * per_map;
        const int row = (int)(in_map / W), w = (int)(in_map - (long long)row * W);
        near_d[g] = dilated_word(seen + (size_t)b * per_map, S, W, row, w, d);
    }
}

// near_d eroded by d at word (row, w) of one map, the pixels outside the domain (row or column 0, beyond the grid) counting as set:
// the closing of `seen`.  The caller keeps (row, w) inside the grid.
__device__ __forceinline__ u64 eroded_word(const u64* __restrict__ near_d, int S, int W, int row, int w, int d) {
    u64 l = ~0ull, c = ~0ull, r = ~0ull;
    const int r0 = row - d < 1 ? 1 : row - d, r1 = row + d > S - 1 ? S - 1 : row + d;       // (row 0 is outside the domain)
    for (int q = r0; q <= r1; ++q) {
        const u64* line = near_d + (size_t)q * W;
        c &= line[w] | (w == 0 ? 1ull : 0ull);                                             // (so is column 0)
        if (w > 0) l &= line[w - 1] | (w == 1 ? 1ull : 0ull);
        if (w + 1 < W) r &= line[w + 1];
    }
    u64 out = c;
    for (int k = 1; k <= d; ++k)
        out &= ((c << k) | (l >> (64 - k))) & ((c >> k) | (r << (64 - k)));
    return out;
}

// the pixels of word (row, w) that lie in the domain (row, column >= 1); 0 outside the grid
__device__ __forceinline__ u64 domain_word(int S, int W, int row, int w) {
    if (row < 1 || row >= S || w < 0 || w >= W) return 0;
    return w == 0 ? ~1ull : ~0ull;
}

// ---- erode: word g of `unknown` = the domain's pixels outside the closing of `seen`
__global__ __launch_bounds__(FR_THREADS) void frontier_erode_kernel(const u64* __restrict__ near_d, long long n_words, int S, int W, int d,
                                                                    u64* __restrict__ unknown) {
    const long long per_map = (long long)S * W;
    for (long long g = (long long)blockIdx.x * FR_THREADS + threadIdx.x; g < n_words; g += (long long)gridDim.x * FR_THREADS) {
        const long long b = g / per_map, in_map = g - b * per_map;
        const int row = (int)(in_map / W), w = (int)(in_map - (long long)row * W);
        const u64 dom = domain_word(S, W, row, w);
        unknown[g] = dom ? dom & ~eroded_word(near_d + (size_t)b * per_map, S, W, row, w, d) : 0ull;
    }
}

// ---- frontier: word g <- free & (an edge neighbour is unknown); out2 where asked for
__global__ __launch_bounds__(FR_THREADS) void frontier_word_kernel(const u64* __restrict__ seen, const u64* __restrict__ occ,
                                                                   const u64* __restrict__ unknown, long long n_words, int S, int W,
                                                                   u64* __restrict__ frontier, float* __restrict__ out2,
                                                                   int unknown_obstacle) {
    const int lane = threadIdx.x & 63;
    const long long per_map = (long long)S * W;
    for (long long g = (long long)blockIdx.x * FR_WAVES + (threadIdx.x >> 6); g < n_words; g += (long long)gridDim.x * FR_WAVES) {
        const long long b = g / per_map, in_map = g - b * per_map;
        const int row = (int)(in_map / W), w = (int)(in_map - (long long)row * W);
        // the neighbours stay inside this map (row 0 and column 0 hold no unknown pixel)
        const u64 u = unknown[g], up = row > 0 ? unknown[g - W] : 0ull, dn = row + 1 < S ? unknown[g + W] : 0ull;
        const u64 lf = w > 0 ? unknown[g - 1] : 0ull, rt = w + 1 < W ? unknown[g + 1] : 0ull;
        const u64 near = up | dn | (u << 1) | (lf >> 63) | (u >> 1) | (rt << 63);
        if (lane == 0) frontier[g] = seen[g] & ~occ[g] & near;
        if (out2) out2[(size_t)g * 64 + lane] = (unknown_obstacle && ((u >> lane) & 1ull)) ? 1.0f : 0.0f;
    }
}

// ---- gain: block = (map, value row, tile of 64 value columns); four neighbouring lanes = one value cell
__global__ __launch_bounds__(FR_GAIN_THREADS) void frontier_gain_kernel(const u64* __restrict__ frontier, int S, int W, int R, int penalty,
                                                                        SectorRows sectors, float* __restrict__ out1) {
    __shared__ u64 rows[FR_LROWS][FR_LWORDS];
    __shared__ u64 masks[8][FR_ROWS];
    const int V = S / 4, tiles = (V + FR_VC - 1) / FR_VC;
    const long long blk = blockIdx.x;
    const int tile = (int)(blk % tiles), g0 = (int)((blk / tiles) % V);
    const long long b = blk / ((long long)tiles * V);
    const int n_q = 2 * R + 1;
    const int row0 = 4 * g0 - R, word0 = 4 * tile - 1;                    // pixel row / word of rows[0][0]; either may be outside
    const u64* map_bits = frontier + (size_t)b * S * W;
    for (int i = threadIdx.x; i < n_q * FR_LWORDS; i += FR_GAIN_THREADS) {
        const int lr = i / FR_LWORDS, lw = i - lr * FR_LWORDS;
        const int pr = row0 + lr, pw = word0 + lw;
        rows[lr][lw] = (pr >= 0 && pr < S && pw >= 0 && pw < W) ? map_bits[(size_t)pr * W + pw] : 0ull;
    }
    for (int i = threadIdx.x; i < 8 * n_q; i += FR_GAIN_THREADS) {
        const int h = i / n_q, q = i - h * n_q;
        const int lo = sectors.lo[h][q], hi = sectors.hi[h][q];
        masks[h][q] = hi >= lo ? (~0ull >> (63 - (hi - lo))) << lo : 0ull;      // hi - lo <= 62
    }
    __syncthreads();
    const int vc = threadIdx.x / FR_PARTS, part = threadIdx.x % FR_PARTS;
    const int g1 = FR_VC * tile + vc;                  // (cells beyond the grid count zeros and store nothing: every lane shuffles)
    // the window of a row starts at pixel column 4 g1 - R = bit 4 vc - R + 64 of the row in LDS: 33 .. 315, words wi and wi + 1 <= 5
    const int start = 4 * vc - R + 64, wi = start >> 6, sh = start & 63;
    int gain[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row's window: bits past 2 R are cut by the masks; never a shift by 64
    auto window = [&](int q) {
        const u64* line = rows[q];
        const u64 lo = line[wi] >> sh;
        return sh ? lo | (line[wi + 1] << (64 - sh)) : lo;
    };
    auto count = [&](u64 win, int q) {
        if (win == 0) return;                          // (most windows are empty)
#pragma unroll
        for (int h = 0; h < 8; ++h) gain[h] += __popcll(win & masks[h][q]);
    };
    for (int q = part; q < n_q; q += 2 * FR_PARTS) {   // two rows' LDS reads in flight at once
        const u64 w0 = window(q), w1 = q + FR_PARTS < n_q ? window(q + FR_PARTS) : 0ull;
        count(w0, q);
        if (w1) count(w1, q + FR_PARTS);
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {                      // the four lanes of a cell are neighbours
        gain[h] += __shfl_xor(gain[h], 1);
        gain[h] += __shfl_xor(gain[h], 2);
    }
    if (g1 >= V) return;
    const int half = V / 2, a0 = g0 > half ? g0 - half : half - g0, a1 = g1 > half ? g1 - half : half - g1;
    const long long pen = (long long)penalty * (a0 > a1 ? a0 : a1);
#pragma unroll
    for (int h = 0; h < 8; ++h)                        // lane `part` of a cell stores headings part and part + 4
        if ((h & (FR_PARTS - 1)) == part) {
            const long long v = gain[h] - pen;
            out1[(((size_t)b * 8 + h) * V + g0) * V + g1] = (float)(v > 0 ? v : 0);
        }
}

// the integer sector rule of utility/frontier.py
bool in_sector(int h, int dy, int dx) {
    static const int dirs[8][2] = {{-1, 0}, {-1, -1}, {0, -1}, {1, -1}, {1, 0}, {1, 1}, {0, 1}, {-1, 1}};
    const int ur = dirs[h][0], uc = dirs[h][1];
    const int t = dy * ur + dx * uc;
    int s = dx * ur - dy * uc;
    if (s < 0) s = -s;
    return t > 0 && (s + t) * (s + t) < 2 * t * t;
}

// the sector masks of radius R as one column interval per heading and row (a cone cut with a disc is convex); false if a row's
// columns are not contiguous (they always are)
bool build_sector_rows(int R, SectorRows* out) {
    for (int h = 0; h < 8; ++h)
        for (int q = 0; q < FR_ROWS; ++q) {
            int lo = 1, hi = 0, n = 0;
            const int dy = q - R;
            if (q <= 2 * R)
                for (int dx = -R; dx <= R; ++dx)
                    if ((dy || dx) && dy * dy + dx * dx <= R * R && in_sector(h, dy, dx)) {
                        if (!n) lo = dx + R;
                        hi = dx + R;
                        ++n;
                    }
            if (n && hi - lo + 1 != n) return false;
            out->lo[h][q] = (unsigned char)lo;
            out->hi[h][q] = (unsigned char)hi;
        }
    return true;
}

}  // namespace

// ... built once per radius and process
bool nbp_sector_rows(int R, NbpSectorRows* out) {
    static std::mutex lock;
    static SectorRows cache[FR_MAX_R + 1];
    static bool built[FR_MAX_R + 1] = {};
    std::lock_guard<std::mutex> guard(lock);
    if (!built[R]) {
        if (!build_sector_rows(R, &cache[R])) return false;
        built[R] = true;
    }
    *out = cache[R];
    return true;
}

namespace {

int check_shape(int B, int S) {
    NBP_RETURN_IF(B < 1 || S < 1, NBP_E_ARG);
    NBP_RETURN_IF(S % 64 != 0, NBP_E_SHAPE);
    return 0;
}

size_t plane_words(int B, int S) { return (size_t)B * S * (S / 64); }

int word_grid(long long n_words) {
    const long long g = nbp_cdiv(n_words, FR_WAVES);
    return (int)(g > FR_MAX_GRID ? FR_MAX_GRID : g);
}

}  // namespace

void nbp_unknown_words_launch(const float* maps6, int B, int S, int dilate, u64* seen, u64* occ, u64* near_d, u64* unknown,
                              hipStream_t stream) {
    const int W = S / 64;
    const size_t n = plane_words(B, S);
    frontier_pack_kernel<<<word_grid((long long)n), FR_THREADS, 0, stream>>>(maps6, (long long)n, S, W, seen, occ);
    frontier_dilate_kernel<<<nbp_ew_grid((long long)n, FR_THREADS), FR_THREADS, 0, stream>>>(seen, (long long)n, S, W, dilate, near_d);
    frontier_erode_kernel<<<nbp_ew_grid((long long)n, FR_THREADS), FR_THREADS, 0, stream>>>(near_d, (long long)n, S, W, dilate, unknown);
}

namespace {

// pack + dilate + erode (nbp_unknown_words_launch) + frontier words (+ out2): what the two entry points share.  ws holds the seen,
// occupied, near_d and (unless the caller wants them) unknown words.
int launch_mask(const float* maps6, int B, int S, int dilate, u64* ws, u64* frontier_bits, u64* unknown_bits, float* out2,
                int unknown_obstacle, hipStream_t stream) {
    const int W = S / 64;
    const size_t n = plane_words(B, S);
    u64 *seen = ws, *occ = ws + n, *near_d = ws + 2 * n, *unknown = unknown_bits ? unknown_bits : ws + 3 * n;
    nbp_unknown_words_launch(maps6, B, S, dilate, seen, occ, near_d, unknown, stream);
    frontier_word_kernel<<<word_grid((long long)n), FR_THREADS, 0, stream>>>(seen, occ, unknown, (long long)n, S, W, frontier_bits, out2,
                                                                             unknown_obstacle);
    return nbp_launch_status();
}

}  // namespace

extern "C" size_t nbp_frontier_workspace_bytes(int B, int S) {
    if (check_shape(B, S)) return 0;
    return 5 * plane_words(B, S) * sizeof(u64);
}

extern "C" int nbp_frontier_mask_u64(const float* maps6, int B, int S, int dilate, unsigned long long* frontier_bits,
                                     unsigned long long* unknown_bits_or_null, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!maps6 || !frontier_bits || !ws, NBP_E_ARG);
    int rc = check_shape(B, S);
    if (rc) return rc;
    NBP_RETURN_IF(dilate < 0 || dilate > FR_MAX_D, NBP_E_ARG);
    NBP_RETURN_IF((((uintptr_t)frontier_bits | (uintptr_t)unknown_bits_or_null | (uintptr_t)ws) & 7) != 0, NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < 4 * plane_words(B, S) * sizeof(u64), NBP_E_WS);
    return launch_mask(maps6, B, S, dilate, (u64*)ws, frontier_bits, unknown_bits_or_null, nullptr, 0, (hipStream_t)stream);
}

extern "C" int nbp_frontier_policy_f32(const float* maps6, int B, int S, int radius, int dilate, int unknown_obstacle,
                                       int distance_penalty, float* out1, float* out2, void* ws, size_t ws_bytes, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!maps6 || !out1 || !out2 || !ws, NBP_E_ARG);
    int rc = check_shape(B, S);
    if (rc) return rc;
    NBP_RETURN_IF(radius < 1 || radius > FR_MAX_R || dilate < 0 || dilate > FR_MAX_D || distance_penalty < 0, NBP_E_ARG);
    NBP_RETURN_IF(((uintptr_t)ws & 7) != 0, NBP_E_SHAPE);
    NBP_RETURN_IF(ws_bytes < 5 * plane_words(B, S) * sizeof(u64), NBP_E_WS);
    SectorRows sectors;
    NBP_RETURN_IF(!nbp_sector_rows(radius, &sectors), NBP_E_ARG);
    const int W = S / 64, V = S / 4;
    u64* bits = (u64*)ws + 4 * plane_words(B, S);
    rc = launch_mask(maps6, B, S, dilate, (u64*)ws, bits, nullptr, out2, unknown_obstacle != 0, (hipStream_t)stream);
    if (rc) return rc;
    // maps go to the gain kernel in chunks whose block count fits a grid dimension
    const long long per_map = (long long)V * nbp_cdiv(V, FR_VC);
    const long long chunk = per_map > (1ll << 24) ? 1 : (1ll << 24) / per_map;      // (2^24 blocks of 256 threads: below 2^32 threads)
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long nb = B - b0 < chunk ? B - b0 : chunk;
        frontier_gain_kernel<<<(unsigned)(nb * per_map), FR_GAIN_THREADS, 0, (hipStream_t)stream>>>(
            bits + (size_t)b0 * S * W, S, W, radius, distance_penalty, sectors, out1 + (size_t)b0 * 8 * V * V);
    }
    return nbp_launch_status();
}
