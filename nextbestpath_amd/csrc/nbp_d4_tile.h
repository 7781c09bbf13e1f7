// nbp_d4_tile.h -- the 64 x 64 tile mover of the D4 kernels (nbp_augment.hip: training batches; nbp_ensemble.hip: the symmetry
// ensemble of the eval forward).
//
// A plane is an n x n window centred on the camera: index i sits at offset (i - n/2) cells from it, so the reflection about the
// camera is i -> n - i (index 0, the half-width bin at the window's far edge, has its mirror image outside the array: the reflected
// plane's index 0 is zero).  An op code is bit 0 = transpose, bit 1 = reflect rows, bit 2 = reflect cols, applied in that order:
//     out[r][c] = A[fr ? n - r : r][fc ? n - c : c],  A = transpose ? in^T : in,  0 where (fr and r == 0) or (fc and c == 0).
//
// A workgroup of 256 threads owns one 64 x 64 output tile.  The source window of the tile (64 rows x at most 68 columns, the
// reflections shift it by one pixel off the 16-byte grid) is read with aligned 16-byte loads along the SOURCE rows into LDS; the
// output is then assembled from LDS four columns at a time along the OUTPUT rows, so a transposing element never touches global
// memory with a stride of n floats per lane.  LDS rows are 81 words apart (81 = 1 mod 16): a wave's 16 float4 columns x 4 rows land
// on distinct banks modulo 64 in both orientations.  n % 4 == 0 and 16-byte aligned planes are the callers' to check.
#ifndef NBP_D4_TILE_H
#define NBP_D4_TILE_H
#include "common.h"

namespace d4 {

constexpr int T = 64;              // output tile side
constexpr int C4 = 17;             // 16-byte columns of the source window (64 + up to 3 floats of alignment slack, + 1)
constexpr int PITCH = 81;          // LDS row pitch in words
constexpr int TILE_WORDS = T * PITCH;

// Fills `tile` with the source window of output tile (R0, C0) of an n x n plane under `op` (not the identity) and returns the
// window's column offset inside its first 16-byte column.  Words whose source lies outside the plane are left as they were: they
// are the mirror images of index n (and of cells beyond the plane), which read4 never uses.  The caller's barrier follows.
__device__ __forceinline__ int load_window(const float* __restrict__ src, int n, int op, int R0, int C0, float* tile, int tid) {
    const bool tr = op & 1, fr = op & 2, fc = op & 4;
    // r' = fr ? n - r : r over the tile's rows, c' likewise: first values of the two (ascending) windows
    const int rp0 = fr ? n - R0 - (T - 1) : R0, cp0 = fc ? n - C0 - (T - 1) : C0;
    const int sr0 = tr ? cp0 : rp0, sc0 = tr ? rp0 : cp0;       // the window in source coordinates
    const int sca = sc0 & ~3;                                   // floor to the 16-byte grid (two's complement: also below zero)
    for (int idx = tid; idx < T * C4; idx += 256) {
        const int rl = idx / C4, j = idx - rl * C4;
        const int sr = sr0 + rl, sc = sca + 4 * j;
        if (sr >= 0 && sr < n && sc >= 0 && sc < n) {           // (n % 4 == 0: a 16-byte column is inside or outside as a whole)
            const float4 v = *(const float4*)(src + (size_t)sr * n + sc);
            float* t = tile + rl * PITCH + 4 * j;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    }
    return sc0 - sca;
}

// The four output values (r, c .. c + 3), r = R0 + rl, c = C0 + cl, of the plane moved by `op`, from the window load_window left.
__device__ __forceinline__ void read4(const float* tile, int op, int coff, int rl, int cl, int r, int c, float o[4]) {
    const bool tr = op & 1, fr = op & 2, fc = op & 4;
    const bool zr = fr && r == 0;
    const int rq = fr ? (T - 1) - rl : rl;                      // r' - rp0
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cq = fc ? (T - 1) - (cl + k) : cl + k;        // c' - cp0
        const float v = tr ? tile[cq * PITCH + rq + coff] : tile[rq * PITCH + cq + coff];
        o[k] = (zr || (fc && c + k == 0)) ? 0.0f : v;           // the mirror image of index n: outside the window
    }
}

// dst tile (R0, C0) = `op` applied to src, both n x n; tile: TILE_WORDS floats of LDS.  Block-uniform arguments but tid.
__device__ __forceinline__ void move_tile(const float* __restrict__ src, float* __restrict__ dst, int n, int op, int R0, int C0,
                                          float* tile, int tid) {
    if (op == 0) {                 // identity: a straight 16-byte copy of the tile (block-uniform branch, no barrier behind it)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, r = R0 + (idx >> 4), c = C0 + 4 * (idx & 15);
            if (r < n && c < n) *(float4*)(dst + (size_t)r * n + c) = *(const float4*)(src + (size_t)r * n + c);
        }
        return;
    }
    const int coff = load_window(src, n, op, R0, C0, tile, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, rl = idx >> 4, cl = 4 * (idx & 15);
        const int r = R0 + rl, c = C0 + cl;
        if (r >= n || c >= n) continue;
        float o[4];
        read4(tile, op, coff, rl, cl, r, c, o);
        *(float4*)(dst + (size_t)r * n + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace d4
#endif
