// nbp_augment.hip -- exact D4 symmetry augmentation of a training batch (include/nbp_hip.h: nbp_augment_batch_f32).
//
// One launch moves the 6 B planes of a batch (5 input maps + the ground-truth layout per sample).  Every plane is an S x S window
// centred on the camera: pixel index i sits at offset (i - S/2) cells from it, so the reflection about the camera is i -> S - i
// (index 0, the half-width bin at the window's far edge, has its mirror image outside the array: the reflected plane's index 0
// is zero).  An op code is bit 0 = transpose, bit 1 = reflect rows, bit 2 = reflect cols, applied in that order:
//     out[r][c] = A[fr ? S - r : r][fc ? S - c : c],  A = transpose ? in^T : in,  0 where (fr and r == 0) or (fc and c == 0).
//
// One workgroup per 64 x 64 output tile; the tile mover (source window through LDS, 16-byte accesses along rows on both sides) is
// nbp_d4_tile.h's, shared with the symmetry ensemble of the eval forward (nbp_ensemble.hip).
#include "nbp_d4_tile.h"

namespace {

__global__ __launch_bounds__(256) void augment_batch_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                            const int* __restrict__ ops, int S, float* __restrict__ x_out,
                                                            float* __restrict__ gt_out) {
    __shared__ float tile[d4::TILE_WORDS];
    const int plane = blockIdx.z, b = plane / 6, ch = plane - 6 * b;
    const size_t SS = (size_t)S * S;
    const float* __restrict__ src = ch < 5 ? x + ((size_t)b * 5 + ch) * SS : gt + (size_t)b * SS;
    float* __restrict__ dst = ch < 5 ? x_out + ((size_t)b * 5 + ch) * SS : gt_out + (size_t)b * SS;
    d4::move_tile(src, dst, S, ops[b] & 7, blockIdx.y * d4::T, blockIdx.x * d4::T, tile, threadIdx.x);
}

}  // namespace

extern "C" int nbp_augment_batch_f32(const float* x, const float* gt, const int* ops_dev, int B, int S, float* x_out, float* gt_out,
                                     void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !gt || !ops_dev || !x_out || !gt_out || B < 1 || S < 1, NBP_E_ARG);
    NBP_RETURN_IF(x_out == x || gt_out == gt || x_out == gt || gt_out == x, NBP_E_ARG);          // out of place only
    NBP_RETURN_IF(S % 16 != 0 || 6ll * B > 65535, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)x_out | (uintptr_t)gt_out) & 15) != 0, NBP_E_SHAPE);
    const int tiles = (S + d4::T - 1) / d4::T;
    augment_batch_kernel<<<dim3(tiles, tiles, 6 * B), 256, 0, (hipStream_t)stream>>>(x, gt, ops_dev, S, x_out, gt_out);
    return nbp_launch_status();
}
