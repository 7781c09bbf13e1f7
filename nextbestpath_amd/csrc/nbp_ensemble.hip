// nbp_ensemble.hip -- the D4 symmetry ensemble of the eval forward (include/nbp_hip.h: nbp_ensemble_expand_f32,
// nbp_ensemble_reduce_f32; definition in float64: utility/augment.py::ensemble_reference).
//
//   expand   x [B,5,S,S] -> x_out [n,B,5,S,S], x_out[k][b] = g_k x[b], g_k = ops[k]: the 5 n B planes in one launch, each 64 x 64
//            output tile by nbp_d4_tile.h's mover (the one nbp_augment.hip uses).
//   reduce   raw1 [n,B,8,V,V], raw2 [n,B,1,S,S] (the network's outputs on the expanded batch) -> out1 [B,8,V,V], out2 [B,1,S,S]:
//            member k is moved back by g_k^-1 and the members are averaged.  g^-1 is g itself except that codes 3 and 5 (the two
//            quarter turns) swap.  A value map also permutes its heading channels: channel heading_map(g^-1)[h] of the moved map is
//            plane h of the member's, so output channel c reads source channel heading_map(g^-1)^-1 (c); the three generators'
//            channel maps are involutions, so the inverse applies them in the opposite order.  A member whose g^-1 reflects rows has
//            nothing to say about row 0 (the mirror image of that row lies outside the window), likewise columns: a cell is divided by
//            the number of members that do reach it, which takes four values per launch (interior, row 0, column 0, corner).
//            One launch: blockIdx.z < B are the obstacle planes (side S), the other 8 B the value planes (side V = S / 4); a
//            workgroup owns a 64 x 64 output tile and takes the n source windows through LDS in turn, accumulating in fp32 registers
//            in the order k = 0 .. n-1.  No atomics: two runs give the same bits.
#include "nbp_d4_tile.h"

namespace {

__device__ __forceinline__ int inverse_op(int op) { return op == 3 ? 5 : op == 5 ? 3 : op; }

// the channel of a member's value map that lands in channel c when the map is moved by g
__device__ __forceinline__ int source_channel(int g, int c) {
    if (g & 4) c = (8 - c) & 7;
    if (g & 2) c = (4 - c) & 7;
    if (g & 1) c = (2 - c) & 7;
    return c;
}

__global__ __launch_bounds__(256) void ensemble_expand_kernel(const float* __restrict__ x, const int* __restrict__ ops, int B, int S,
                                                              float* __restrict__ x_out) {
    __shared__ float tile[d4::TILE_WORDS];
    const int plane = blockIdx.z, k = plane / (5 * B);           // x_out plane (k, b, ch) <- x plane (b, ch)
    const size_t SS = (size_t)S * S;
    d4::move_tile(x + (size_t)(plane - 5 * B * k) * SS, x_out + (size_t)plane * SS, S, ops[k] & 7, blockIdx.y * d4::T,
                  blockIdx.x * d4::T, tile, threadIdx.x);
}

__global__ __launch_bounds__(256) void ensemble_reduce_kernel(const float* __restrict__ raw1, const float* __restrict__ raw2,
                                                              const int* __restrict__ ops, int n, int B, int S,
                                                              float* __restrict__ out1, float* __restrict__ out2) {
    __shared__ float tile[d4::TILE_WORDS];
    const int p = blockIdx.z;
    const bool value = p >= B;
    const int side = value ? S / 4 : S;
    const int R0 = blockIdx.y * d4::T, C0 = blockIdx.x * d4::T;
    if (R0 >= side || C0 >= side) return;                       // the grid is the obstacle planes': block-uniform, no barrier yet
    const int b = value ? (p - B) >> 3 : p, ch = value ? (p - B) & 7 : 0;
    const size_t PP = (size_t)side * side;
    const int tid = threadIdx.x;
    float acc[4][4] = {};
    int n_rows = 0, n_cols = 0, n_either = 0;                   // members that do not reach row 0 / column 0 / the corner
    for (int k = 0; k < n; ++k) {
        const int g = inverse_op(ops[k] & 7);
        n_rows += (g >> 1) & 1; n_cols += (g >> 2) & 1; n_either += (g & 6) != 0;
        const float* __restrict__ src = value ? raw1 + (((size_t)k * B + b) * 8 + source_channel(g, ch)) * PP
                                              : raw2 + ((size_t)k * B + b) * PP;
        if (g == 0) {                                           // block-uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i, r = R0 + (idx >> 4), c = C0 + 4 * (idx & 15);
                if (r >= side || c >= side) continue;
                const float4 v = *(const float4*)(src + (size_t)r * side + c);
                acc[i][0] += v.x; acc[i][1] += v.y; acc[i][2] += v.z; acc[i][3] += v.w;
            }
            continue;
        }
        const int coff = d4::load_window(src, side, g, R0, C0, tile, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, rl = idx >> 4, cl = 4 * (idx & 15);
            const int r = R0 + rl, c = C0 + cl;
            if (r >= side || c >= side) continue;
            float o[4];
            d4::read4(tile, g, coff, rl, cl, r, c, o);          // 0 where the member does not reach
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += o[j];
        }
        __syncthreads();                                        // the next member's window overwrites the tile
    }
    float* __restrict__ dst = value ? out1 + ((size_t)b * 8 + ch) * PP : out2 + (size_t)b * PP;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = R0 + (idx >> 4), c = C0 + 4 * (idx & 15);
        if (r >= side || c >= side) continue;
        const float rest = (float)(n - (r == 0 ? n_rows : 0));                                   // columns >= 1
        const float first = (float)(n - (r == 0 ? n_either : n_cols));                           // column 0
        *(float4*)(dst + (size_t)r * side + c) =
            make_float4(acc[i][0] / (c == 0 ? first : rest), acc[i][1] / rest, acc[i][2] / rest, acc[i][3] / rest);
    }
}

}  // namespace

extern "C" int nbp_ensemble_expand_f32(const float* x, int B, int S, const int* ops_dev, int n, float* x_out, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!x || !ops_dev || !x_out || B < 1 || S < 1 || n < 1 || n > 8, NBP_E_ARG);
    NBP_RETURN_IF(x_out == x, NBP_E_ARG);                                                        // out of place only
    NBP_RETURN_IF(S % 16 != 0 || 5ll * n * B > 65535, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)x | (uintptr_t)x_out) & 15) != 0, NBP_E_SHAPE);
    const int tiles = (S + d4::T - 1) / d4::T;
    ensemble_expand_kernel<<<dim3(tiles, tiles, 5 * n * B), 256, 0, (hipStream_t)stream>>>(x, ops_dev, B, S, x_out);
    return nbp_launch_status();
}

extern "C" int nbp_ensemble_reduce_f32(const float* raw1, const float* raw2, int B, int S, const int* ops_dev, int n, float* out1,
                                       float* out2, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!raw1 || !raw2 || !ops_dev || !out1 || !out2 || B < 1 || S < 1 || n < 1 || n > 8, NBP_E_ARG);
    NBP_RETURN_IF(out1 == raw1 || out2 == raw2 || out1 == raw2 || out2 == raw1 || out1 == out2, NBP_E_ARG);   // out of place only
    NBP_RETURN_IF(S % 16 != 0 || 9ll * B > 65535, NBP_E_SHAPE);
    NBP_RETURN_IF((((uintptr_t)raw1 | (uintptr_t)raw2 | (uintptr_t)out1 | (uintptr_t)out2) & 15) != 0, NBP_E_SHAPE);
    const int tiles = (S + d4::T - 1) / d4::T;
    ensemble_reduce_kernel<<<dim3(tiles, tiles, 9 * B), 256, 0, (hipStream_t)stream>>>(raw1, raw2, ops_dev, n, B, S, out1, out2);
    return nbp_launch_status();
}
