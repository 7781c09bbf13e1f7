// nbp_depth_noise.hip -- the seeded depth-sensor noise model (include/nbp_hip.h: nbp_depth_noise_f32, nbp_depth_noise_batch_f32;
// the definition, which this file equals bit for bit, is nextbestpath_amd/utility/depth_noise.py).
//
// Clean frame -> noisy frame, out of place (the edge test reads clean neighbours).  A frame's noise depends on (seed, frame id,
// pixel) only: counter-based words, so there is no generator state, no workspace and no atomics.  One lane owns 4 consecutive
// pixels of a frame (blockIdx.z = frame): 16-byte loads and stores when the frames lie on the 16-byte grid and W % 4 == 0 (then a
// lane's pixels share a row and the rows above and below are quads too), 4-byte accesses for any other H, W >= 1.  Neighbour rows
// are plain loads, issued only when the edge test is on.  8 H W bytes of traffic per frame; the work is ~90 integer operations
// per pixel: a streaming kernel whose cost at the rollouts' 256 x 456 frames is its launch.
#include "common.h"

#pragma clang fp contract(off)      // the five fp32 operations of the definition, each rounded on its own

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_ITEMS = 12;                       // the step's group stages chunk at 12 items (nbp_sim.hip: STEP_BATCH) ...
constexpr int DN_FRAMES = 4 * DN_ITEMS;            // ... of <= 4 frames each

struct NoiseSpec { float sigma_base, sigma_quad, z_min, edge_threshold; unsigned drop_thr; };
struct NoiseBatch { const float* clean[DN_FRAMES]; float* out[DN_FRAMES]; unsigned seed[DN_FRAMES]; unsigned frame[DN_FRAMES]; };

__device__ __forceinline__ unsigned mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned word(unsigned p, unsigned k, unsigned key) { return mix(mix((8u * p + k) ^ key) + key); }

// the noisy value of valid clean depth z at pixel p, or -1 when the dropout word drops it
__device__ __forceinline__ float noisy(float z, unsigned p, unsigned key, const NoiseSpec& sp) {
    unsigned s = 0;
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) s = __builtin_amdgcn_sad_u8(word(p, k, key), 0u, s);      // + the word's 4 bytes
    const float g = ((float)s - 2040.0f) * 0.0033829375f;
    float t = z * z;
    float a = sp.sigma_quad * t;
    a = sp.sigma_base + a;
    const float d = a * g;
    float zn = z + d;
    zn = fmaxf(zn, sp.z_min);
    if (sp.drop_thr != 0u && word(p, 4u, key) < sp.drop_thr) zn = -1.0f;
    return zn;
}

// is valid depth z a flying pixel against neighbour depth nb (a background neighbour does not count)
__device__ __forceinline__ bool far_apart(float z, float nb, float thr) { return nb > -1.0f && fabsf(z - nb) > thr; }

// ONE body for both launch forms: the 4 pixels from p0 of one [H][W] frame
__device__ __forceinline__ void noise_quad(const float* __restrict__ clean, float* __restrict__ out, int H, int W, unsigned HW, unsigned p0,
                                           unsigned key, const NoiseSpec& sp, bool vec) {
    const bool edge = sp.edge_threshold > 0.0f;
    const float thr = sp.edge_threshold;
    if (vec) {                                     // W % 4 == 0: p0 .. p0 + 3 lie in one row, every quad is whole
        const unsigned row = p0 / (unsigned)W, col = p0 - row * (unsigned)W;
        const f32x4 c = *(const f32x4*)(clean + p0);
        bool drop[4] = {false, false, false, false};
        if (edge) {
            const float none = -1.0f;              // (a background neighbour: never counts)
            f32x4 up = {none, none, none, none}, dn = up;
            if (row > 0) up = *(const f32x4*)(clean + p0 - W);
            if (row + 1 < (unsigned)H) dn = *(const f32x4*)(clean + p0 + W);
            const float left = col > 0 ? clean[p0 - 1] : none, right = col + 4 < (unsigned)W ? clean[p0 + 4] : none;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = c[j], l = j > 0 ? c[j - 1] : left, r = j < 3 ? c[j + 1] : right;
                drop[j] = far_apart(z, l, thr) || far_apart(z, r, thr) || far_apart(z, up[j], thr) || far_apart(z, dn[j], thr);
            }
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (c[j] > -1.0f && !drop[j]) ? noisy(c[j], p0 + j, key, sp) : -1.0f;
        *(f32x4*)(out + p0) = o;
        return;
    }
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const unsigned p = p0 + j;
        if (p >= HW) return;
        const float z = clean[p];
        float o = -1.0f;
        if (z > -1.0f) {
            bool drop = false;
            if (edge) {
                const unsigned row = p / (unsigned)W, col = p - row * (unsigned)W;
                drop = (col > 0 && far_apart(z, clean[p - 1], thr)) || (col + 1 < (unsigned)W && far_apart(z, clean[p + 1], thr)) ||
                       (row > 0 && far_apart(z, clean[p - W], thr)) || (row + 1 < (unsigned)H && far_apart(z, clean[p + W], thr));
            }
            if (!drop) o = noisy(z, p, key, sp);
        }
        out[p] = o;
    }
}

__device__ __forceinline__ unsigned frame_key(unsigned seed, unsigned frame) { return mix(mix(seed ^ 0x9E3779B9u) + frame); }

// n consecutive frames of one camera: frame blockIdx.z has id first_frame + blockIdx.z (wrapping)
__global__ __launch_bounds__(DN_THREADS) void depth_noise_kernel(const float* __restrict__ clean, float* __restrict__ out, int H, int W,
                                                                 unsigned HW, unsigned seed, unsigned first_frame, NoiseSpec sp, int vec) {
    const unsigned p0 = 4u * (blockIdx.x * DN_THREADS + threadIdx.x);
    if (p0 >= HW) return;
    const size_t off = (size_t)blockIdx.z * HW;
    noise_quad(clean + off, out + off, H, W, HW, p0, frame_key(seed, first_frame + blockIdx.z), sp, vec != 0);
}

// frame blockIdx.z of the batch: its own pointers, seed and id, all kernel arguments
__global__ __launch_bounds__(DN_THREADS) void depth_noise_batch_kernel(NoiseBatch b, int H, int W, unsigned HW, NoiseSpec sp, int vec) {
    const unsigned p0 = 4u * (blockIdx.x * DN_THREADS + threadIdx.x);
    if (p0 >= HW) return;
    const unsigned f = blockIdx.z;
    noise_quad(b.clean[f], b.out[f], H, W, HW, p0, frame_key(b.seed[f], b.frame[f]), sp, vec != 0);
}

// NBP_E_* of the arguments the two forms share, 0 when they are fine
int check_spec(int H, int W, float sigma_base, float sigma_quad, float z_min, float edge_threshold) {
    NBP_RETURN_IF(H < 1 || W < 1, NBP_E_ARG);
    NBP_RETURN_IF((long long)H * W > (1ll << 29), NBP_E_SHAPE);                 // 8 p + k is a 32-bit counter
    NBP_RETURN_IF(!(sigma_base >= 0.f) || !(sigma_quad >= 0.f) || !(z_min > 0.f) || !(edge_threshold >= 0.f), NBP_E_ARG);
    return 0;
}

bool overlap(const float* a, const float* b, size_t n) { return a < b + n && b < a + n; }

}  // namespace

extern "C" int nbp_depth_noise_f32(const float* clean, float* out, int n, int H, int W, unsigned seed, unsigned first_frame,
                                   float sigma_base, float sigma_quad, float z_min, unsigned drop_thr, float edge_threshold, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(!clean || !out || n < 1, NBP_E_ARG);
    int rc = check_spec(H, W, sigma_base, sigma_quad, z_min, edge_threshold);
    if (rc) return rc;
    NBP_RETURN_IF(n > 65535, NBP_E_SHAPE);
    const unsigned HW = (unsigned)H * (unsigned)W;
    NBP_RETURN_IF(overlap(clean, out, (size_t)n * HW), NBP_E_ARG);               // out of place: the edge test reads clean neighbours
    const NoiseSpec sp = {sigma_base, sigma_quad, z_min, edge_threshold, drop_thr};
    const int vec = W % 4 == 0 && (((uintptr_t)clean | (uintptr_t)out) & 15) == 0;
    dim3 grid((unsigned)nbp_cdiv(nbp_cdiv(HW, 4), DN_THREADS), 1, (unsigned)n);
    depth_noise_kernel<<<grid, DN_THREADS, 0, (hipStream_t)stream>>>(clean, out, H, W, HW, seed, first_frame, sp, vec);
    return nbp_launch_status();
}

extern "C" int nbp_depth_noise_batch_f32(int n, const float* const* clean, float* const* out, const unsigned* seeds, const unsigned* frames,
                                         int H, int W, float sigma_base, float sigma_quad, float z_min, unsigned drop_thr,
                                         float edge_threshold, void* stream) {
    NBP_ENTER();
    NBP_RETURN_IF(n < 1 || !clean || !out || !seeds || !frames, NBP_E_ARG);
    NBP_RETURN_IF(n > DN_FRAMES, NBP_E_SHAPE);
    int rc = check_spec(H, W, sigma_base, sigma_quad, z_min, edge_threshold);
    if (rc) return rc;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const NoiseSpec sp = {sigma_base, sigma_quad, z_min, edge_threshold, drop_thr};
    NoiseBatch b;
    int vec = W % 4 == 0;
    for (int f = 0; f < n; ++f) {
        NBP_RETURN_IF(!clean[f] || !out[f], NBP_E_ARG);
        for (int g = 0; g < n; ++g) NBP_RETURN_IF(clean[g] && overlap(clean[g], out[f], HW), NBP_E_ARG);
        for (int g = 0; g < f; ++g) NBP_RETURN_IF(overlap(out[g], out[f], HW), NBP_E_ARG);
        if ((((uintptr_t)clean[f] | (uintptr_t)out[f]) & 15) != 0) vec = 0;
    }
    for (int f = 0; f < DN_FRAMES; ++f) {
        const int q = f < n ? f : 0;
        b.clean[f] = clean[q]; b.out[f] = out[q]; b.seed[f] = seeds[q]; b.frame[f] = frames[q];
    }
    dim3 grid((unsigned)nbp_cdiv(nbp_cdiv(HW, 4), DN_THREADS), 1, (unsigned)n);
    depth_noise_batch_kernel<<<grid, DN_THREADS, 0, (hipStream_t)stream>>>(b, H, W, HW, sp, vec);
    return nbp_launch_status();
}
