// nbp_augment.hip -- exact D4 symmetry augmentation of a training batch (include/nbp_hip.h: nbp_augment_batch_f32).
//
// One launch moves the 6 B planes of a batch (5 input maps + the ground-truth layout per sample).  Every plane is an S x S window
// centred on the camera: pixel index i sits at offset (i - S/2) cells from it, so the reflection about the camera is i -> S - i
// (index 0, the half-width bin at the window's far edge, has its mirror image outside the array: the reflected plane's index 0
// is zero).  An op code is bit 0 = transpose, bit 1 = reflect rows, bit 2 = reflect cols, applied in that order:
//     out[r][c] = A[fr ? S - r : r][fc ? S - c : c],  A = transpose ? in^T : in,  0 where (fr and r == 0) or (fc and c == 0).
//
// A workgroup of 256 threads writes one 64 x 64 output tile.  The source window of the tile (64 rows x at most 68 columns, the
// reflections shift it by one pixel off the 16-byte grid) is read with aligned 16-byte loads along the SOURCE rows into LDS; the
// output is then assembled from LDS and written with 16-byte stores along the OUTPUT rows, so a transposing element never touches
// global memory with a stride of S floats per lane.  LDS rows are 81 words apart (81 = 1 mod 16): a wave's 16 float4 columns x 4
// rows land on distinct banks modulo 64 in both orientations.
#include "common.h"

namespace {

constexpr int AUG_T = 64;          // output tile side
constexpr int AUG_C4 = 17;         // 16-byte columns of the source window (64 + up to 3 floats of alignment slack, + 1)
constexpr int AUG_PITCH = 81;      // LDS row pitch in words

__global__ __launch_bounds__(256) void augment_batch_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                            const int* __restrict__ ops, int S, float* __restrict__ x_out,
                                                            float* __restrict__ gt_out) {
    __shared__ float tile[AUG_T * AUG_PITCH];
    const int plane = blockIdx.z, b = plane / 6, ch = plane - 6 * b;
    const size_t SS = (size_t)S * S;
    const float* __restrict__ src = ch < 5 ? x + ((size_t)b * 5 + ch) * SS : gt + (size_t)b * SS;
    float* __restrict__ dst = ch < 5 ? x_out + ((size_t)b * 5 + ch) * SS : gt_out + (size_t)b * SS;
    const int op = ops[b] & 7;
    const int R0 = blockIdx.y * AUG_T, C0 = blockIdx.x * AUG_T;
    const int tid = threadIdx.x;

    if (op == 0) {                 // identity: a straight 16-byte copy of the tile (block-uniform branch, no barrier behind it)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, r = R0 + (idx >> 4), c = C0 + 4 * (idx & 15);
            if (r < S && c < S) *(float4*)(dst + (size_t)r * S + c) = *(const float4*)(src + (size_t)r * S + c);
        }
        return;
    }
    const bool tr = op & 1, fr = op & 2, fc = op & 4;
    // r' = fr ? S - r : r over the tile's rows, c' likewise: first values of the two (ascending) windows
    const int rp0 = fr ? S - R0 - (AUG_T - 1) : R0, cp0 = fc ? S - C0 - (AUG_T - 1) : C0;
    const int sr0 = tr ? cp0 : rp0, sc0 = tr ? rp0 : cp0;       // the window in source coordinates
    const int sca = sc0 & ~3;                                   // floor to the 16-byte grid (two's complement: also below zero)
    for (int idx = tid; idx < AUG_T * AUG_C4; idx += 256) {
        const int rl = idx / AUG_C4, j = idx - rl * AUG_C4;
        const int sr = sr0 + rl, sc = sca + 4 * j;
        if (sr >= 0 && sr < S && sc >= 0 && sc < S) {           // (S % 4 == 0: a 16-byte column is inside or outside as a whole)
            const float4 v = *(const float4*)(src + (size_t)sr * S + sc);
            float* t = tile + rl * AUG_PITCH + 4 * j;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    }
    __syncthreads();
    const int coff = sc0 - sca;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, rl = idx >> 4, cl = 4 * (idx & 15);
        const int r = R0 + rl, c = C0 + cl;
        if (r >= S || c >= S) continue;
        const bool zr = fr && r == 0;
        const int rq = fr ? (AUG_T - 1) - rl : rl;              // r' - rp0
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cq = fc ? (AUG_T - 1) - (cl + k) : cl + k;        // c' - cp0
            const float v = tr ? tile[cq * AUG_PITCH + rq + coff] : tile[rq * AUG_PITCH + cq + coff];
            o[k] = (zr || (fc && c + k == 0)) ? 0.0f : v;       // the mirror image of index S: outside the window
        }
        *(float4*)(dst + (size_t)r * S + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace

extern "C" int nbp_augment_batch_f32(const float* x, const float* gt, const int* ops_dev, int B, int S, float* x_out, float* gt_out,
                                     void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !gt || !ops_dev || !x_out || !gt_out || B < 1 || S < 1, NBP_E_ARG);
    NBP_RETURN_IF(x_out == x || gt_out == gt || x_out == gt || gt_out == x, NBP_E_ARG);          // out of place only
    NBP_RETURN_IF(S % 16 != 0 || 6ll * B > 65535, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)x_out | (uintptr_t)gt_out) & 15) != 0, NBP_E_SHAPE);
    const int tiles = (S + AUG_T - 1) / AUG_T;
    augment_batch_kernel<<<dim3(tiles, tiles, 6 * B), 256, 0, (hipStream_t)stream>>>(x, gt, ops_dev, S, x_out, gt_out);
    return nbp_launch_status();
}
