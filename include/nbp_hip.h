/* nbp_hip.h -- C ABI of libnbp_hip.so: the MI355X (gfx950) hot path of NextBestPath.
 *
 * The reference (shiyao-li/NextBestPath) is pure Python and has no native boundary; the
 * functions below are what a maintainer's ctypes binding replaces the cited torch /
 * PyTorch3D / trimesh call sites with (INTEGRATION.md shows the stubs).  Citations are
 * relative to the reference repository root.
 *
 * Conventions
 *  - every function returns 0 on success, a negative NBP_E_* code on an argument error
 *    (nothing is launched / written) or a positive hipError_t if a launch failed;
 *  - every pointer is caller-owned DEVICE memory unless the name ends in _host;
 *  - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; pass
 *    torch.cuda.current_stream().cuda_stream); no function synchronises or allocates device
 *    memory: scratch comes in through (ws, ws_bytes) sized by the matching *_workspace_bytes;
 *  - activations inside the network are NHWC fp32; the public tensors keep the reference's
 *    NCHW layout ([B,5,S,S] in, [B,8,S/4,S/4] and [B,1,S,S] out);
 *  - no exceptions cross the boundary, no global mutable state besides the explicit handle;
 *  - this project's own ctypes binding (nextbestpath_amd/_lib.py) reads its signatures from the declarations below, so a new
 *    entry point is declared here, defined in csrc/, and is bound.  For that a declaration has the form
 *    `<ret> nbp_<name>(<params>);` with int, unsigned, long long, unsigned long long, float, double, size_t (or a void return)
 *    and pointers only: no other scalar type, array parameter or function pointer, and comments in the C form.
 */
#ifndef NBP_HIP_H
#define NBP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBP_E_ARG      (-1)  /* null pointer / bad shape / bad enum                       */
#define NBP_E_WS       (-2)  /* workspace too small                                       */
#define NBP_E_SHAPE    (-3)  /* shape not supported by the kernels (e.g. S % 16 != 0)     */

/* ---------------------------------------------------------------- library info */
/* ABI version of this header; bumped on any signature change. */
int nbp_abi_version(void);
/* Writes gcnArchName / CU count of the current device (host strings/ints). */
int nbp_device_info(char* arch_host, int arch_len, int* cu_count_host);
/* The library's launch plans (tile choice, split-K bounds, fusions) are compile-time constants.  Their A/B switches (NBP_*
 * environment variables) are honoured ONLY when the process sets NBP_TUNING=1; an inherited environment
 * never changes results.  nbp_tuning_active: 1 when the opt-in is set.  nbp_tuning_report: writes "NAME=value,..." of the
 * switches read so far whose value differs from the default into buf_host (truncated to len - 1) and returns their number. */
int nbp_tuning_active(void);
int nbp_tuning_report(char* buf_host, int len);
/* Kernel symbol (as a profiler demangles it, without "void" / the anonymous namespace / the argument list) that convolution tile
 * id `tile` (nbp_layer_timing.tile) was most recently launched as in this process; returns its length, 0 if that tile id has not
 * been launched yet.  The launchers build the text from their own template arguments. */
int nbp_tile_kernel_symbol(int tile, char* buf_host, int len);

/* ================================================================ A1: NBP network
 * Replaces NBP.forward, next_best_path/networks/nbp_model.py:110-160 (and the layer
 * classes :8-62) for inference (module.eval(): BatchNorm uses running statistics).
 *
 * Canonical order of the 48 convolutions (index -> reference parameter prefix):
 *   0..9   Conv{1..5}.conv.{0,3}
 *   then for decoder d=1 (levels L=5,4) and d=2 (levels L=5,4,3,2), six per level:
 *          Up{L}_d.up.1, Att{L}_d.W_g.0, Att{L}_d.W_x.0, Att{L}_d.psi.0,
 *          Up_conv{L}_d.conv.0, Up_conv{L}_d.conv.3
 *   i.e. 10..21 decoder 1, 22..45 decoder 2, then 46 Final1, 47 Final2.0
 */
#define NBP_N_CONV 48

typedef struct nbp_weights nbp_weights;   /* opaque: host-side table of pointers into `packed` */

/* Bytes of device memory the packed fp32 weights + folded affine terms need. */
size_t nbp_packed_weights_bytes(void);

/* Re-lays the 48 OIHW fp32 weight tensors into the K-chunked layout the implicit-GEMM
 * kernels stream ([c_in/32][tap][c_out][32]) inside caller memory `packed`, and copies the
 * per-output-channel epilogue terms: out = act(acc * scale + shift).
 *   w[i]      OIHW fp32 weight of conv i (device)
 *   scale[i]  [c_out] fp32 (device): gamma/sqrt(var+eps) (1 when the conv has no BatchNorm)
 *   shift[i]  [c_out] fp32 (device): (bias-mean)*scale+beta
 * For the attention pair (W_g, W_x) the two 1x1 convolutions are fused into one GEMM over
 * the concatenated K = [g | x]: their `scale` is multiplied into the packed weights and the
 * caller passes shift[W_g] = shift_g + shift_x (shift[W_x] is ignored).
 * On success *handle_out is a host object to pass to nbp_forward_f32; free it with
 * nbp_free_weights (which never touches `packed`). */
int nbp_pack_weights(const void* const* w_host_array, const void* const* scale_host_array,
                     const void* const* shift_host_array, void* packed, size_t packed_bytes,
                     void* stream, nbp_weights** handle_out);
void nbp_free_weights(nbp_weights* handle);

size_t nbp_forward_workspace_bytes(int B, int S);

/* x [B,5,S,S] -> out1 [B,8,S/4,S/4] (linear), out2 [B,1,S,S] (sigmoid); S % 16 == 0. */
int nbp_forward_f32(const nbp_weights* handle, const float* x, int B, int S, float* out1,
                    float* out2, void* ws, size_t ws_bytes, void* stream);

/* Profiling twin of nbp_forward_f32: brackets every launch group with hipEvents on `stream`,
 * SYNCHRONISES the stream, and fills timings_host[0..*n_entries_host) (one entry per layer, in
 * launch order; `ms` of a split-K layer includes its reduce kernel).  tile: id of the convolution
 * kernel used (see nbp_conv_igemm_f32), -1 for the other kernels.  Not re-entrant. */
typedef struct nbp_layer_timing {
    char name[48];
    double flops;      /* 2*M*N*K */
    float ms;
    int tile, split_k;
    long long M;
    int N, K;
} nbp_layer_timing;
int nbp_forward_timed_f32(const nbp_weights* handle, const float* x, int B, int S, float* out1,
                          float* out2, void* ws, size_t ws_bytes, void* stream,
                          nbp_layer_timing* timings_host, int max_entries, int* n_entries_host);

/* FLOPs (2*MAC over the 48 convolutions) of one forward at batch B, size S. */
double nbp_forward_flops(int B, int S);

/* ---- bf16 variant (BASELINE.json configs[4]: 512x512 grids, 8 rollouts per GPU in one forward).
 * Same network and same fp32 in/out tensors as nbp_forward_f32 (ref nbp_model.py:110-160); inside, activations
 * are NHWC bf16, the 3x3 / attention-gate weights are bf16, accumulation and every epilogue (folded BatchNorm,
 * ReLU, sigmoid, psi gate) are fp32, and each stored activation is rounded once (nearest even).  It cannot
 * meet the 1e-4 fp32 tolerance (bf16 has 8 mantissa bits); tests/test_gpu_bf16.py states its tolerance.
 * nbp_pack_weights_bf16 takes exactly the inputs of nbp_pack_weights (`packed` of nbp_packed_weights_bytes_bf16()). */
int nbp_pack_weights_bf16(const void* const* w_host_array, const void* const* scale_host_array,
                          const void* const* shift_host_array, void* packed, size_t packed_bytes,
                          void* stream, nbp_weights** handle_out);
size_t nbp_packed_weights_bytes_bf16(void);   /* `packed` of nbp_pack_weights_bf16: the common pack + the up_conv parity filters */
size_t nbp_forward_workspace_bytes_bf16(int B, int S);
/* up_conv parity filters in bf16 for nbp_conv_igemm_bf16 with tile 12 / 13 (8 x 32 low-resolution tiles x 128 / 64 channels;
 * ups must be 1, C1 0): dst [parity][C/64][4 taps][N][64] bf16 = 32 N C bytes. */
int nbp_pack_upconv_weight_bf16(const float* w_oihw, int N, int C, unsigned short* dst, void* stream);
int nbp_forward_bf16(const nbp_weights* handle, const float* x, int B, int S, float* out1,
                     float* out2, void* ws, size_t ws_bytes, void* stream);
int nbp_forward_timed_bf16(const nbp_weights* handle, const float* x, int B, int S, float* out1,
                           float* out2, void* ws, size_t ws_bytes, void* stream,
                           nbp_layer_timing* timings_host, int max_entries, int* n_entries_host);

/* ---- fp32 forward with the 3x3 convolutions on the 16-bit matrix pipe ("split" path, nbp_split.hip).
 * Tensors, accumulation and epilogues are fp32 exactly as in nbp_forward_f32; inside the 3x3 kernels every fp32 operand is
 * scaled by a power of two taken from its tensor's max |x| and cut into two fp16 pieces (hi + lo = s x up to 2^-23), and
 * the product is evaluated as three exact fp16 MFMAs (the dropped lo x lo is < 2^-22 of the product): error against fp64
 * not above the fp32 MFMA chain's at 5.3x its matrix rate; up_conv layers run as four 2x2 parity
 * convolutions of the low-resolution input, the attention gates' joint 1x1 GEMM on the same split scheme.  Layers the split
 * kernels do not take (images that are not multiples of 16 x 32 / 16 x 16 pixels, psi, the heads) run nbp_forward_f32's kernels.  The handle
 * of nbp_pack_weights_split (`packed` of nbp_packed_weights_bytes_split()) also serves nbp_forward_f32. */
size_t nbp_packed_weights_bytes_split(void);
int nbp_pack_weights_split(const void* const* w_host_array, const void* const* scale_host_array,
                           const void* const* shift_host_array, void* packed, size_t packed_bytes, void* stream,
                           nbp_weights** handle_out);
size_t nbp_forward_workspace_bytes_split(int B, int S);
int nbp_forward_split_f32(const nbp_weights* handle, const float* x, int B, int S, float* out1, float* out2, void* ws,
                          size_t ws_bytes, void* stream);
int nbp_forward_timed_split_f32(const nbp_weights* handle, const float* x, int B, int S, float* out1, float* out2,
                                void* ws, size_t ws_bytes, void* stream, nbp_layer_timing* timings_host,
                                int max_entries, int* n_entries_host);
/* One 3x3 layer of that path (stride 1, zero padding 1; src1 / ups as nbp_conv_igemm_f32).
 * nbp_pack_conv_weight_split: planes [chunk of 16 channels][tap][hi|lo][k half][N][8] fp16 (4 bytes per weight; zero the
 * buffer first when C < c_total) scaled by 2^(14 - floor(log2 max|w|)); wamax_out = device word that receives max |w * scale|
 * (float bits).  c_off must be 0 (one scale per layer).
 * nbp_conv3x3_split_f32: images of 16 x 32 pixel tiles with N % 64 == 0, or of 16 x 16 pixel tiles with N % 128 == 0; channel
 * counts multiples of 32; NBP_E_SHAPE otherwise.  amax_in = 64 device words (256 B) whose maximum is max |x| over src0 and
 * src1 (float bits; a bound is enough), NULL = computed here (one more pass over the inputs); amax_out (or NULL) = 64 words
 * that receive max |out| by atomicMax spread over the words: zero them before, and hand them to the consumer layer as its
 * amax_in.  nbp_amax_f32 is that pass on its own (same 64-word convention).  split_k 0 = automatic;
 * ws >= nbp_conv_split_workspace_bytes. */
int nbp_pack_conv_weight_split(const float* w_oihw, int N, int C, int ksize, const float* scale_or_null, int c_off,
                               int c_total, void* dst_planes, void* wamax_out, void* stream);
int nbp_amax_f32(const float* x, long long n, void* amax_inout, void* stream);
/* up_conv (x2 nearest upsample + 3x3 convolution, nbp_model.py:25-33) as four 2x2 convolutions of the low-resolution input, one
 * per output parity, with pre-summed weights (16 tap-products per low-resolution pixel instead of 36).
 * nbp_pack_upconv_weight_split: planes [parity][chunk of 16][4 taps][hi|lo][k half][N][8] fp16 (64 N C bytes); the sums are
 * formed in double and split directly.
 * nbp_upconv3x3_split_f32: src [B,H/2,W/2,C] -> out [B,H,W,N]; the low-resolution image must tile (H/2 % 16 == 0 and W/2 % 32 == 0
 * with N % 64 == 0, or W/2 % 16 == 0 with N % 128 == 0), NBP_E_SHAPE otherwise; other arguments as nbp_conv3x3_split_f32. */
int nbp_pack_upconv_weight_split(const float* w_oihw, int N, int C, void* dst_planes, void* wamax_out, void* stream);
int nbp_upconv3x3_split_f32(const float* src, int C, int B, int H, int W, const void* planes_up, const void* wamax_up, int N,
                            const float* scale, const float* shift, int relu, float* out, const void* amax_in_or_null,
                            void* amax_out_or_null, int split_k, void* ws, size_t ws_bytes, void* stream);
size_t nbp_conv_split_workspace_bytes(int B, int H, int W, int N, int split_k);
/* The same for split_k = 0 as the planner will actually run the layer (C = C0 + C1 input channels): its split-K count is
 * returned through split_k_out (may be NULL; 0 = the layer is not taken by the split kernel).  Slices exist for occupancy
 * (small grids) and for accuracy: an accumulation chain is bounded to NBP_SPLIT_MAX_K_SMALL (576) products where a slice of
 * the output is <= 64 MB and to NBP_SPLIT_MAX_K (2304) elsewhere, so that the result's distance to the exact sum does not
 * grow with the batch size. */
size_t nbp_conv_split_planned_workspace_bytes(int B, int H, int W, int C, int N, int ups, int* split_k_out);
/* ... for a split_k request: 0 = the planner with its accuracy-driven chain bound (the eval forward), < 0 = the planner by
 * occupancy only (the training step), > 0 = as given.  The same request goes to nbp_conv3x3_split_f32 / nbp_upconv3x3_split_f32. */
size_t nbp_conv_split_planned_workspace_bytes_k(int B, int H, int W, int C, int N, int ups, int split_k, int* split_k_out);
int nbp_conv3x3_split_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                          const void* w_planes, const void* wamax, int N, const float* scale, const float* shift, int relu,
                          float* out, const void* amax_in_or_null, void* amax_out_or_null, int split_k, void* ws,
                          size_t ws_bytes, void* stream);
/* Weight gradient of Conv1.conv.0 (nbp_model.py:66: 5 -> 64 channels, 3x3) straight from the NCHW network input x [B,5,H,W] and
 * dy [B,H,W,64] (NHWC): dw [64][5][3][3].  H % 8 == 0, W % 32 == 0 (else NBP_E_SHAPE: the caller pads the input to 64 channels and
 * takes nbp_conv_wgrad_split_f32).  The forward of the layer is nbp_conv_first_f32. */
size_t nbp_conv_first_wgrad_workspace_bytes(void);
int nbp_conv_first_wgrad_f32(const float* x_nchw, int B, int H, int W, const float* dy, float* dw, void* ws, size_t ws_bytes, void* stream);
/* Every weight pack of a training step in two launches.  descs_dev: n records on the device, each
 *   { const float* w; uint16_t* planes; uint16_t* planes_t; uint32_t* wamax; int32 N, C, kind, pad; }   (nbp_prepack_desc_bytes() = 48)
 * kind 0: 3x3 layer w [N][C][3][3] -> planes of nbp_pack_conv_weight_split and planes_t of nbp_pack_conv_weight_split_dgrad;
 * kind 1: 1x1 layer w [N][C] -> planes (ksize 1) and planes_t of nbp_pack_conv1x1_weight_split_dgrad;
 * kind 2: up_conv layer -> planes of nbp_pack_upconv_weight_split and planes_t of nbp_pack_upconv_weight_split_dgrad.
 * planes_t may be null.  wamax: the record's own word inside wamax_words [n] (zeroed by the call).  N % 16 == 0, C % 16 == 0. */
int nbp_prepack_weights_split(const void* descs_dev, int n, void* wamax_words, void* stream);
int nbp_prepack_desc_bytes(void);
/* Training-step forms of nbp_pack_conv_weight_split / _dgrad: `_prezeroed` takes a max-|w| word the caller zeroed (no memset launch),
 * `_dgrad_known` reuses the word the forward's pack of the same weights left (the data-gradient planes hold the same values): one
 * launch instead of three. */
int nbp_pack_conv_weight_split_prezeroed(const float* w_oihw, int N, int C, int ksize, int c_total, void* dst_planes,
                                         void* wamax_zeroed, void* stream);
int nbp_pack_conv_weight_split_dgrad_known(const float* w_oihw, int N, int C, int c_total, void* dst_planes, const void* wamax_known,
                                           void* stream);
/* Data gradient of an up_conv layer (nbp_model.py:25-33: x2 nearest upsample + 3x3 convolution, C -> N channels) in the parity form of
 * nbp_upconv3x3_split_f32: dx [B,H,W,C] at the LOW resolution straight from dy [B,2H,2W,N] -- 16 tap-products per low-resolution pixel
 * instead of the 36 of the full-resolution 3x3 data gradient followed by a 2x2 sum.  nbp_pack_upconv_weight_split_dgrad: 32 N C fp16
 * from the layer's own OIHW weight; scale / shift: C ones / zeros; amax_in: 64-word max-|dy| slot; ws: nbp_upconv_split_dgrad_workspace_bytes.
 * NBP_E_SHAPE when the low-resolution image does not tile (H % 16, W % 32 with C % 64, or W % 16 with C % 128). */
int nbp_pack_upconv_weight_split_dgrad(const float* w_oihw, int N, int C, void* dst_planes, void* wamax_out, void* stream);
size_t nbp_upconv_split_dgrad_workspace_bytes(int B, int H, int W, int N, int C);
int nbp_upconv3x3_split_dgrad_f32(const float* dy, int N, int B, int H, int W, const void* planes, const void* wamax, int C,
                                  const float* scale, const float* shift, float* dx, const void* amax_in, void* amax_out_or_null,
                                  void* ws, size_t ws_bytes, void* stream);
/* Weight gradient of the same layer in parity form: dW [N][C][3][3] from the LOW-resolution input x [B,Hs,Ws,C] and dy [B,2Hs,2Ws,N] as
 * 16 tap-GEMMs over M / 4 pixels (four parities x 2 x 2 taps) folded into the 3x3 filter by the reduce kernel; C % 64 == 0, N % 64 == 0,
 * (Ws % 32 == 0 and Hs % 2 == 0) or (Ws % 16 == 0 and Hs % 4 == 0), else NBP_E_SHAPE.  amax_x / amax_y: 64-word max-|.| slots. */
size_t nbp_upconv_wgrad_split_workspace_bytes(int B, int Hs, int Ws, int C, int N);
int nbp_upconv_wgrad_split_f32(const float* x, int C, int B, int Hs, int Ws, const float* dy, int N, float* dw,
                               const void* amax_x, const void* amax_y, void* ws, size_t ws_bytes, void* stream);
/* 1x1 convolution on the same scheme (training: Attention_block.W_g / W_x, nbp_model.py:44-53, and their data gradients):
 * out [M][N] = src [M][C] W * scale + shift, C % 32 == 0, N % 32 == 0.  w_planes / wamax: nbp_pack_conv_weight_split with ksize 1
 * (forward) or nbp_pack_conv1x1_weight_split_dgrad (dx = dy W^T from the layer's own [N][C] weight).  amax_in: 64-word max-|src| slot. */
int nbp_conv1x1_split_f32(const float* src, int C, long long M, const void* w_planes, const void* wamax, int N,
                          const float* scale, const float* shift, int relu, float* out, const void* amax_in, void* stream);
int nbp_pack_conv1x1_weight_split_dgrad(const float* w_nc, int N, int C, void* dst_planes, void* wamax_out, void* stream);
/* Training: planes of the DATA-GRADIENT convolution of a 3x3 layer (dx = conv3x3(dy, w'), w'[c][n][tap] = w[n][c][8 - tap]; autograd
 * of nn.Conv2d, nbp_model.py:14-33) straight from the layer's weights w [N][C][3][3]: C rows, N input channels padded to c_total */
int nbp_pack_conv_weight_split_dgrad(const float* w_oihw, int N, int C, int c_total, void* dst_planes, void* wamax_out, void* stream);

/* Training: the same convolution (and its up_conv form), whose epilogue also leaves the column sums of the output and of its
 * squares for the BatchNorm behind it (nextbestpath_amd/networks/training.py: ConvFn -> BNFn; the reference's nn.Sequential of
 * Conv2d + BatchNorm2d, nbp_model.py:14-33): bn_part receives *bn_rows rows of [2][N] doubles -- at most
 * nbp_conv_bn_part_rows(B, H, W) rows -- finalised by nbp_bn_train_forward_part4_f32 without another pass over the tensor.
 * *bn_rows = 0: this launch did not take them (split-K or half-height tiles); the caller's BatchNorm reads the tensor itself. */
int nbp_conv_bn_part_rows(int B, int H, int W);
int nbp_conv3x3_split_bn_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                             const void* w_planes, const void* wamax, int N, const float* scale, const float* shift, int relu,
                             float* out, const void* amax_in_or_null, void* amax_out_or_null, int split_k, void* ws,
                             size_t ws_bytes, double* bn_part, int* bn_rows, void* stream);
int nbp_upconv3x3_split_bn_f32(const float* src, int C, int B, int H, int W, const void* planes_up, const void* wamax_up, int N,
                               const float* scale, const float* shift, int relu, float* out, const void* amax_in_or_null,
                               void* amax_out_or_null, int split_k, void* ws, size_t ws_bytes, double* bn_part, int* bn_rows,
                               void* stream);
/* ---- One-piece ("_h1") forms of the training step's split kernels (NBP.train_precision = "fp16"; nbp_split.hip, template
 * parameter ONE).  Each takes the arguments of the entry point without the suffix.  Operands are scaled by the same per-tensor power
 * of two as the split path (max |x| in [2^14, 2^15)) and rounded ONCE to fp16, hi = fp16(s x); every product is one
 * v_mfma_f32_32x32x16_f16 (exact in the fp32 accumulator) instead of three; the epilogues, scales, amax slots and split-K plans are
 * the split path's.  Weight planes: [chunk of 16][tap][k half][rows][8] fp16 of the hi pieces alone (half the bytes of the
 * two-piece planes); the convolutions take only planes from the `_h1` packs. */
int nbp_pack_conv_weight_split_h1(const float* w_oihw, int N, int C, int ksize, const float* scale_or_null, int c_off,
                                  int c_total, void* dst_planes, void* wamax_out, void* stream);
int nbp_pack_conv_weight_split_prezeroed_h1(const float* w_oihw, int N, int C, int ksize, int c_total, void* dst_planes,
                                            void* wamax_zeroed, void* stream);
int nbp_pack_conv_weight_split_dgrad_h1(const float* w_oihw, int N, int C, int c_total, void* dst_planes, void* wamax_out, void* stream);
int nbp_pack_conv_weight_split_dgrad_known_h1(const float* w_oihw, int N, int C, int c_total, void* dst_planes, const void* wamax_known,
                                              void* stream);
int nbp_pack_upconv_weight_split_h1(const float* w_oihw, int N, int C, void* dst_planes, void* wamax_out, void* stream);
int nbp_pack_upconv_weight_split_dgrad_h1(const float* w_oihw, int N, int C, void* dst_planes, void* wamax_out, void* stream);
int nbp_pack_conv1x1_weight_split_dgrad_h1(const float* w_nc, int N, int C, void* dst_planes, void* wamax_out, void* stream);
int nbp_prepack_weights_split_h1(const void* descs_dev, int n, void* wamax_words, void* stream);
int nbp_conv3x3_split_f32_h1(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                             const void* w_planes, const void* wamax, int N, const float* scale, const float* shift, int relu,
                             float* out, const void* amax_in_or_null, void* amax_out_or_null, int split_k, void* ws,
                             size_t ws_bytes, void* stream);
int nbp_conv3x3_split_bn_f32_h1(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                                const void* w_planes, const void* wamax, int N, const float* scale, const float* shift, int relu,
                                float* out, const void* amax_in_or_null, void* amax_out_or_null, int split_k, void* ws,
                                size_t ws_bytes, double* bn_part, int* bn_rows, void* stream);
int nbp_upconv3x3_split_f32_h1(const float* src, int C, int B, int H, int W, const void* planes_up, const void* wamax_up, int N,
                               const float* scale, const float* shift, int relu, float* out, const void* amax_in_or_null,
                               void* amax_out_or_null, int split_k, void* ws, size_t ws_bytes, void* stream);
int nbp_upconv3x3_split_bn_f32_h1(const float* src, int C, int B, int H, int W, const void* planes_up, const void* wamax_up, int N,
                                  const float* scale, const float* shift, int relu, float* out, const void* amax_in_or_null,
                                  void* amax_out_or_null, int split_k, void* ws, size_t ws_bytes, double* bn_part, int* bn_rows,
                                  void* stream);
int nbp_upconv3x3_split_dgrad_f32_h1(const float* dy, int N, int B, int H, int W, const void* planes, const void* wamax, int C,
                                     const float* scale, const float* shift, float* dx, const void* amax_in, void* amax_out_or_null,
                                     void* ws, size_t ws_bytes, void* stream);
int nbp_conv1x1_split_f32_h1(const float* src, int C, long long M, const void* w_planes, const void* wamax, int N,
                             const float* scale, const float* shift, int relu, float* out, const void* amax_in, void* stream);
int nbp_upconv_wgrad_split_f32_h1(const float* x, int C, int B, int Hs, int Ws, const float* dy, int N, float* dw,
                                  const void* amax_x, const void* amax_y, void* ws, size_t ws_bytes, void* stream);
int nbp_conv_wgrad_split_f32_h1(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W, int ksize,
                                const float* dy, int N, int c_real, int n_real, float* dw, const void* amax0_or_null,
                                const void* amax1_or_null, const void* amaxy_or_null, void* ws, size_t ws_bytes, void* stream);
/* BatchNorm2d training forward from those partial sums (zero_row = C zeros): finalize + normalise, x is read once */
int nbp_bn_train_forward_part4_f32(const float* x, long long M, int C, const float* gamma, const float* beta, float eps,
                                   float momentum, float* running_mean, float* running_var, int relu, float* mean, float* invstd,
                                   float* y, void* amax_out, double* stat_out, int stat_doubles, const double* part, int rows,
                                   const float* zero_row, void* stream);
/* Single bf16 layer: as nbp_conv_igemm_f32 with bf16 (uint16 storage) NHWC sources / output, C0, C1 multiples
 * of 64, w_packed from nbp_pack_conv_weight_bf16 ([(c_off+c)/64][tap][N][64] bf16), fp32 scale / shift. */
int nbp_conv_igemm_bf16(const unsigned short* src0, int C0, const unsigned short* src1, int C1, int ups,
                        int B, int H, int W, int ksize, const unsigned short* w_packed, int N,
                        const float* scale, const float* shift, int relu, unsigned short* out,
                        int split_k, int tile, void* ws, size_t ws_bytes, void* stream);
size_t nbp_conv_igemm_bf16_workspace_bytes(int B, int H, int W, int N, int split_k);
int nbp_pack_conv_weight_bf16(const float* w_oihw, int N, int C, int ksize, const float* scale_or_null,
                              int c_off, int c_total, unsigned short* dst, void* stream);
/* Element-wise conversions (round to nearest even), for tests and callers holding fp32 maps. */
int nbp_f32_to_bf16(const float* in, long long n, unsigned short* out, void* stream);
int nbp_bf16_to_f32(const unsigned short* in, long long n, float* out, void* stream);

/* ---- single layers (same kernels the forward uses; exported for layer-level parity tests)
 * Implicit-GEMM convolution on NHWC fp32, k in {1,3}, stride 1, "same" padding:
 *   input channels [0,C0) come from src0, [C0,C0+C1) from src1 (fused torch.cat, ref :128);
 *   ups != 0 reads the sources through a x2 nearest upsample (fused nn.Upsample, ref :27):
 *   sources are then [B,H/2,W/2,C];  C0,C1 multiples of 32 (C1 may be 0), N multiple of 32.
 *   w_packed: layout produced by nbp_pack_conv_weight.  out [B,H,W,N] = act(acc*scale+shift).
 *   split_k >= 1 splits the K loop over blockIdx.z (ws must hold split_k*B*H*W*N floats);
 *   split_k == 0 lets the library choose.  tile: 0 = auto; 1..5 = implicit-GEMM workgroup tiles (pixels x
 *   channels) 128x128, 256x64, 256x32, 128x64, 64x128; 6 / 7 = the halo-tile kernel (3x3 only, H % 8 == 0,
 *   W % 32 == 0) with 128 / 64 output channels per workgroup, whose split-K slices are whole channel chunks.
 *   Ids reported by the timing twins for the other paths: 10 / 11 = split-path 16-row tiles (plain / up_conv parity form), 15 / 16 = the
 *   same on 8 x 32-pixel tiles (launches with fewer 16-row tiles than CUs); nbp_conv_igemm_bf16 also takes 12 / 13 (parity form) and
 *   14 (3x3, H % 16 == 0, W % 32 == 0, N % 64 == 0, no split-K: 16 x 32 pixels x 64 channels, weights in registers). */
int nbp_conv_igemm_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H,
                       int W, int ksize, const float* w_packed, int N, const float* scale,
                       const float* shift, int relu, float* out, int split_k, int tile, void* ws,
                       size_t ws_bytes, void* stream);
size_t nbp_conv_igemm_workspace_bytes(int B, int H, int W, int N, int split_k);

/* OIHW [N][C][k][k] -> packed [(c_off+c)/32][tap][N][32]; optional per-n scale multiply.
 * c_total = total input channels of the fused K (c_off + C <= c_total). */
int nbp_pack_conv_weight(const float* w_oihw, int N, int C, int ksize, const float* scale_or_null,
                         int c_off, int c_total, float* dst, void* stream);

/* Conv1.conv.0: NCHW [B,5,H,W] -> NHWC [B,H,W,64], 3x3, act(acc*scale+shift), ReLU.
 * w is the raw OIHW [64,5,3,3] tensor. */
int nbp_conv_first_f32(const float* x_nchw, int B, int H, int W, const float* w_oihw,
                       const float* scale, const float* shift, float* out_nhwc, void* stream);
/* The same layer without the ReLU (training: the train-mode BatchNorm that follows takes conv + bias); H % 8 == 0, W % 32 == 0. */
int nbp_conv_first_linear_f32(const float* x_nchw, int B, int H, int W, const float* w_oihw, const float* scale,
                              const float* shift, float* out_nhwc, void* stream);
/* nn.MaxPool2d(2,2) on NHWC (ref :68). */
int nbp_maxpool2_nhwc_f32(const float* in, int B, int H, int W, int C, float* out, void* stream);
/* Attention gate tail (ref :59-62): psi = sigmoid((q . w_psi) * s + t) per pixel,
 * out = x * psi.  q [M,F] (already ReLU'd g1+x1), x/out [M,C]. */
int nbp_psi_gate_f32(const float* q, int F, const float* w_psi, const float* s_t2, const float* x,
                     int C, long long M, float* out, void* stream);
/* Final 1x1 convolutions (ref :85,105-106): NHWC [B,H,W,C] -> NCHW [B,n_out,H,W],
 * out = act(acc*scale+shift), act = sigmoid if `sigmoid` else identity.  n_out <= 8. */
int nbp_final_1x1_f32(const float* in, int B, int H, int W, int C, const float* w_oc, int n_out,
                      const float* scale, const float* shift, int sigmoid, float* out_nchw,
                      void* stream);
/* Layout helpers (tests / training path). */
int nbp_nchw_to_nhwc_f32(const float* in, int B, int C, int H, int W, float* out, void* stream);
int nbp_nhwc_to_nchw_f32(const float* in, int B, int C, int H, int W, float* out, void* stream);

/* ================================================================ A4-A7: map accumulation
 * World points -> agent-centred top-down count images.
 * Index rule (next_best_path/utility/utils.py:198-223, :160-164):
 *   v0 = -(p.z - c.z), v1 = -(p.x - c.x)                       (utils.py:166-196, R = I)
 *   i0 = rint((v0 - lo) * (S / (hi - lo))) , i1 likewise        (fp32, half-to-even)
 *   counted iff 0 <= i0,i1 < S;  out[i0*S + i1] += 1
 */
/* utils.py:166-196 transform_points_to_n_pieces (no_rotation=True): [N,3] -> [N,2]. */
int nbp_transform_points_f32(const float* points, long long N, float cx, float cy, float cz,
                             float* out_2d, void* stream);
/* utils.py:198-223 map_points_to_n_imgs: pts2d [n,m,2] -> out [n,S0,S1] fp32 counts.
 * `out` is zeroed by this call. */
int nbp_map_points_to_imgs_f32(const float* pts2d, int n, long long m, int S0, int S1, float lo,
                               float hi, float* out, void* stream);
/* utils.py:160-164 get_point_position_in_the_img for K points: -> [2,K] int64 (no bounds
 * check, like the reference). */
int nbp_point_position_i64(const float* pts2d, long long K, int S0, int S1, float lo, float hi,
                           long long* out_2xK, void* stream);
/* One fused pass over the accumulated cloud (nbp_planning.py:114-127 slab split +
 * :172-183 full / height-band projections): out [6,S,S] fp32, zeroed by this call:
 *   ch 0..3  height slabs: bin = #{k : bounds[k] < p.y} - 1 (torch.bucketize, right=False)
 *            counted iff 0 <= bin < 4 (n_bounds is len(y_bins)-1, normally 4, at most 8)
 *   ch 4     points that fall in no slab (so that ch0+..+ch4 = projection of ALL points)
 *   ch 5     points with  band_lo < p.y < band_hi   (the reference's +-0.1 height band)
 * N_dev_or_null: when non-null the point count is read from device memory (the rollout keeps the
 * cloud size on the device so the step loop never synchronises) and N is only an upper bound. */
int nbp_map_accumulate_f32(const float* points, long long N, const long long* N_dev_or_null, float cx,
                           float cy, float cz, const float* bounds_host, int n_bounds, float band_lo,
                           float band_hi, int S, float lo, float hi, float* out6, void* stream);
/* The "observation -> network input" stage of one exploration step (nbp_planning.py:114-137) in one call:
 * nbp_map_accumulate_f32 into out6, the trajectory channel (camera positions so far, transformed like the cloud:
 * (-(z - cz), -(x - cx)), counted per cell as nbp_map_points_to_imgs_f32 does) into net_in5[4], and
 * net_in5[0..3] = out6[0..3]; net_in5 = one [5,S,S] map of the network's input batch.  traj_pts = device history of
 * camera positions with n_traj_old valid points; traj_fresh_host = up to 8 new positions (host, passed in the kernel
 * arguments), appended to traj_pts[n_traj_old ..] by the same launch.  Two memsets, one kernel, one copy. */
int nbp_step_maps_f32(const float* points, long long N, const long long* N_dev_or_null, float cx, float cy,
                      float cz, const float* bounds_host, int n_bounds, float band_lo, float band_hi, int S,
                      float lo, float hi, float* traj_pts, int n_traj_old, const float* traj_fresh_host,
                      int n_traj_fresh, float* out6, float* net_in5, void* stream);
/* The same for the n <= 16 rollouts of a lock-step group in ONE kernel launch (two memsets, one kernel, one strided copy
 * instead of n times that): the step's kernels are latency-bound -- one workgroup per CU, a chain of dependent round trips --
 * so a group costs one such chain.  Rollout r writes out6_all[r] of [n][6][S][S] and net_in_all[r] of [n][5][S][S]; the other
 * arrays are HOST arrays of n entries (points / N_dev / traj_pts: device pointers; N_cap: an upper bound of the cloud size,
 * it sizes the grid; poses_xyz [n][3]; bounds [n][8]; band_lo_hi [n][2]; traj_fresh [n][24]).  Results are identical to n
 * calls of nbp_step_maps_f32. */
int nbp_step_maps_batch_f32(int n, const float* const* points, const long long* N_cap, const long long* const* N_dev,
                            const float* poses_xyz_host, const float* bounds_host, const int* n_bounds,
                            const float* band_lo_hi_host, int S, float lo, float hi, float* const* traj_pts,
                            const int* n_traj_old, const float* traj_fresh_host, const int* n_traj_fresh,
                            float* out6_all, float* net_in_all, void* stream);
/* ---- Tile-binned shadow copy of a rollout's cloud (round 4).  The six maps are a translated window of the world, so the map build
 * can run on points grouped by (x, z) tile: one workgroup per 2048-point PAGE of a tile on a dense 16 x 16-cell x 6-channel
 * histogram in LDS, tiles outside the +-40 window never read.  The canonical cloud (append order) is untouched; the store holds a
 * second copy of every point, filed when a map build first sees it.  Maps are bit-identical to nbp_step_maps_f32's (integer counts).
 *   nbp_cloud_bins_bytes      bytes of the store for a scene whose (x, z) extent is [lo_xz, hi_xz] and a cloud of `capacity` points
 *                             (2.5-unit tiles with one tile of margin; 0 = bad arguments)
 *   nbp_cloud_bins_geometry   the same plan as numbers: {nx, nz, max_pages}, {x0, z0, tile}
 *   nbp_cloud_bins_init       empties the store (256-byte aligned): call it whenever the cloud is reset to zero points
 *   nbp_step_maps_binned_f32  nbp_step_maps_f32 on the store, two launches: points [n_binned, N) of `points` are filed into their
 *                             tiles' pages, then the maps are built from the pages (every point is counted pre-aggregated per tile:
 *                             a fused form that counted the new points with one global atomic each cost the lock-step 5 %).
 *                             page_bound = page workgroups to launch (max_pages is always enough; fewer only cost time: they
 *                             stride over every page that exists).  traj_pts and net_in5 may both be NULL: only out6 is produced.
 *                             Points that cannot be filed (outside the tile grid, page pool exhausted) are kept in an index list
 *                             and counted with direct atomics; if that list overflows too (65536 entries) header word 2 (error)
 *                             becomes non-zero and every later build counts the whole cloud directly: slower, never wrong.
 *   nbp_step_maps_binned_batch_f32  the same for the n <= 16 rollouts of a lock-step group (stores[n], page_bound[n]: HOST arrays).
 * Store header (device, int32 words): 0 n_pages, 1 n_overflow, 2 error, 3 ticket, 4-5 n_binned (int64). */
size_t nbp_cloud_bins_bytes(const float* lo_xz_host, const float* hi_xz_host, long long capacity);
int nbp_cloud_bins_geometry(const float* lo_xz_host, const float* hi_xz_host, long long capacity, int* nx_nz_maxpages_host,
                            float* x0_z0_tile_host);
int nbp_cloud_bins_init(void* store, size_t store_bytes, const float* lo_xz_host, const float* hi_xz_host, long long capacity,
                        void* stream);
int nbp_step_maps_binned_f32(void* store, int page_bound, const float* points, long long N, const long long* N_dev_or_null,
                             float cx, float cy, float cz, const float* bounds_host, int n_bounds, float band_lo, float band_hi,
                             int S, float lo, float hi, float* traj_pts, int n_traj_old, const float* traj_fresh_host,
                             int n_traj_fresh, float* out6, float* net_in5, void* stream);
/* nbp_step_maps_binned_f32 as ONE launch (round 6): the page build alone, for a store whose points were filed by the launch that
 * appended them to the cloud and whose outputs that launch cleared (nbp_unproject_append_filed_f32 with the same store, zero6 = out6,
 * zero1 = net_in5 + 4 S^2).  Same arguments, same maps.  Points the store has not seen (appended by any other route since) are still
 * counted -- directly, slowly -- so a caller's bookkeeping slip costs time, never points. */
int nbp_step_maps_prefiled_f32(void* store, int page_bound, const float* points, long long N, const long long* N_dev_or_null,
                               float cx, float cy, float cz, const float* bounds_host, int n_bounds, float band_lo, float band_hi,
                               int S, float lo, float hi, float* traj_pts, int n_traj_old, const float* traj_fresh_host,
                               int n_traj_fresh, float* out6, float* net_in5, void* stream);
int nbp_step_maps_binned_batch_f32(int n, void* const* stores, const int* page_bound, const float* const* points,
                                   const long long* N_cap, const long long* const* N_dev, const float* poses_xyz_host,
                                   const float* bounds_host, const int* n_bounds, const float* band_lo_hi_host, int S, float lo,
                                   float hi, float* const* traj_pts, const int* n_traj_old, const float* traj_fresh_host,
                                   const int* n_traj_fresh, float* out6_all, float* net_in_all, void* stream);
/* ---- The other latency-bound stages of an exploration step for the rollouts of a lock-step group (n <= 12; coverage: n <= 16),
 * one launch per kernel instead of n.  Every array argument is a HOST array of n entries holding device pointers / scalars;
 * results are identical to n single calls (tests/test_gpu_rollout.py).
 * nbp_coverage_count_planned_batch_f32: nbp_coverage_count_planned_f32 per item (bbox_lo / bbox_hi: [n][3]).
 * nbp_unproject_append_shaded_batch_f32: nbp_unproject_append_shaded_f32 per item for n_frames <= 4 frames each (H W % 4 == 0);
 *   depth / zface: [n][n_frames] pointers, one per FRAME ([H][W] each; a ring's frames need not be adjacent);
 *   cams12_host [n][n_frames][12]; zface / verts / faces / vcolors / cloud_rgb may be NULL (or hold NULLs): depth only;
 *   counts2[r]: 2 n_frames ints (valid, kept per frame); ws[r] >= nbp_unproject_workspace_bytes(n_frames, H, W) each.
 * nbp_raster_zface_batch_f32: nbp_raster_zface_f32 per item (each its own mesh) for n_frames <= 4 views each;
 *   ws[r] >= nbp_raster_workspace_bytes(n_faces[r], n_frames, H, W, 0). */
int nbp_coverage_count_planned_batch_f32(int n, void* const* plans, const int* G, float threshold, const float* bbox_lo_host,
                                         const float* bbox_hi_host, const float* const* pc3, const long long* N,
                                         const long long* const* N_dev, const long long* sample_k, const unsigned* seed,
                                         const unsigned* epoch, int* const* count_accum, int* const* m_out, void* stream);
int nbp_unproject_append_shaded_batch_f32(int n, const float* const* depth, const void* const* zface, const float* const* verts,
                                          const int* const* faces, const float* const* vcolors, const float* cams12_host,
                                          int n_frames, int H, int W, float tan_half_fov, float fov_range,
                                          double gathering_factor, const unsigned* seeds, float ambient, int* const* counts2,
                                          float* const* cloud, float* const* cloud_rgb, long long* const* cloud_count,
                                          const long long* capacity, void* const* ws, size_t ws_bytes_each, void* stream);
int nbp_raster_zface_batch_f32(int n, const float* const* verts, const int* n_verts, const int* const* faces, const int* n_faces,
                               const float* cams12_host, int n_frames, int H, int W, float tan_half_fov, float z_clip,
                               float* const* zbuf, void* const* zface, void* const* ws, const size_t* ws_bytes, void* stream);

/* ================================================================ A14-A17: simulator
 * PyTorch3D / trimesh conventions restated (third-party; parity with the libraries unpinned):
 * cameras are HOST arrays [n][12] fp32 = R row-major (9) then T (3) with X_view = X_world R + T;
 * n <= 8: they travel in the kernel arguments, so a step never blocks on a host->device copy. */

/* Camera.compute_partial_point_cloud (macarons/utility/macarons_utils.py:2811-2847) for n_frames
 * depth maps at once, appended to a device-resident cloud:
 *   valid  = (mask ? mask != 0 : depth > -1) && depth < fov_range            (mu:2825-2828)
 *   n_keep = int(n_valid * gathering_factor)                                  (mu:2836)
 *   kept   = the first n_keep entries of a seeded pseudo-random permutation of the valid pixels
 *            (stands in for torch.randperm, mu:2837; see perm_index in csrc/common.h)
 *   point  = un-projection of (ndc_x(col), ndc_y(row), depth) through the FoV camera (mu:2788-2809)
 * counts2[f] = {n_valid, n_keep}; points land at cloud[*cloud_count + sum_{g<f} n_keep_g + j];
 * *cloud_count is advanced on the device (clamped to capacity). */
size_t nbp_unproject_workspace_bytes(int n_frames, int H, int W);
int nbp_unproject_append_f32(const float* depth, const unsigned char* mask_or_null, const float* cams12_host,
                             int n_frames, int H, int W, float tan_half_fov, float fov_range,
                             double gathering_factor, unsigned seed, int* counts2, float* cloud,
                             long long* cloud_count, long long capacity, void* ws, size_t ws_bytes,
                             void* stream);

/* Camera.capture_image's depth output (mu:2743-2786): zbuf [n_frames,H,W] = view-space z of the
 * nearest face through each pixel centre (perspective-correct, faces clipped at z_clip), -1 where
 * no face.  Faces are binned in two levels (8x8-pixel tiles inside 64x64-pixel coarse tiles) into lists with room for
 * every face: no face is ever dropped (the reference renders with max_faces_per_bin = 500000,
 * macarons/testers/scene.py:440-446).  bin_cap and overflow_flag are kept for ABI compatibility and ignored.
 * Every rasteriser entry point (zbuf, rgbz, zface, zface_batch) returns NBP_E_ARG for z_clip <= 0: depths are merged by atomicMin on
 * their bit patterns, which orders positive floats only. */
size_t nbp_raster_workspace_bytes(int n_faces, int n_frames, int H, int W, int bin_cap);
int nbp_raster_zbuf_f32(const float* verts, int n_verts, const int* faces, int n_faces,
                        const float* cams12_host, int n_frames, int H, int W, float tan_half_fov,
                        float z_clip, int bin_cap, float* zbuf, int* overflow_flag, void* ws,
                        size_t ws_bytes, void* stream);

/* The same render with colours (mu:2743-2763): rgb [n_frames,H,W,3] = ambient x barycentric interpolation of the winning
 * face's vertex colours vcolors3 [V,3] (SoftPhongShader under AmbientLights on a TexturesVertex mesh), white background,
 * then torchvision's adjust_contrast(contrast_factor) (identity for 1); zbuf as above.  ws >= nbp_raster_rgb_workspace_bytes. */
size_t nbp_raster_rgb_workspace_bytes(int n_faces, int n_frames, int H, int W);
int nbp_raster_rgbz_f32(const float* verts, int n_verts, const int* faces, int n_faces, const float* vcolors3,
                        const float* cams12_host, int n_frames, int H, int W, float tan_half_fov, float z_clip,
                        float ambient, float contrast_factor, float* zbuf, float* rgb, void* ws, size_t ws_bytes,
                        void* stream);
/* nbp_unproject_append_f32 that also appends the colours of the kept pixels (rgb [n_frames,H,W,3]) to cloud_rgb
 * [capacity,3] at the same indices (compute_partial_point_cloud with images, mu:2840-2845). */
int nbp_unproject_append_rgb_f32(const float* depth, const unsigned char* mask_or_null, const float* rgb,
                                 const float* cams12_host, int n_frames, int H, int W, float tan_half_fov,
                                 float fov_range, double gathering_factor, unsigned seed, int* counts2,
                                 float* cloud, float* cloud_rgb, long long* cloud_count, long long capacity,
                                 void* ws, size_t ws_bytes, void* stream);

/* Deferred shading (the step loop's form of the colour render): the rasteriser also returns zface [n_frames,H,W] u64 =
 * (depth bits << 32 | nearest face), ~0 for background; colours are then evaluated only where they are consumed --
 * nbp_shade_image_f32 gives the whole rgb image (contrast_factor must be 1: a contrast change needs the eager
 * nbp_raster_rgbz_f32), nbp_unproject_append_shaded_f32 shades just the kept pixels (about 5 %) while appending them.
 * Both rebuild the face record with the rasteriser's arithmetic: colours are bit-identical to nbp_raster_rgbz_f32's. */
int nbp_raster_zface_f32(const float* verts, int n_verts, const int* faces, int n_faces, const float* cams12_host,
                         int n_frames, int H, int W, float tan_half_fov, float z_clip, float* zbuf, void* zface,
                         void* ws, size_t ws_bytes, void* stream);
int nbp_shade_image_f32(const void* zface, const float* verts, const int* faces, const float* vcolors3,
                        const float* cams12_host, int n_frames, int H, int W, float tan_half_fov, float ambient,
                        float contrast_factor, float* rgb, void* stream);
int nbp_unproject_append_shaded_f32(const float* depth, const unsigned char* mask_or_null, const void* zface,
                                    const float* verts, const int* faces, const float* vcolors3,
                                    const float* cams12_host, int n_frames, int H, int W, float tan_half_fov,
                                    float fov_range, double gathering_factor, unsigned seed, float ambient,
                                    int* counts2, float* cloud, float* cloud_rgb, long long* cloud_count,
                                    long long capacity, void* ws, size_t ws_bytes, void* stream);
/* The three calls above in one (by which colour source is given: none, rgb [n_frames,H,W,3], or zface + verts + faces + vcolors3)
 * that also FILES every appended point into the cloud's tile-binned store (nbp_cloud_bins_init; the point is in registers anyway)
 * and, when zero6 / zero1 are given, clears the 6 S^2 / S^2 floats the map build behind it accumulates into: that build is then
 * nbp_step_maps_prefiled_f32 -- one launch instead of two (round 6).  It files only while the store is in step with the cloud
 * (header n_binned == *cloud_count at entry); otherwise the points stay unfiled and the next build counts them directly.
 * Needs the three-launch form (H W % 4 == 0, 16-byte aligned frames): NBP_E_SHAPE otherwise.  Replaces the same reference lines as
 * nbp_unproject_append_f32 (mu:2788-2847) + the scatter's bookkeeping (next_best_path/testers/nbp_planning.py:114-127). */
int nbp_unproject_append_filed_f32(const float* depth, const unsigned char* mask_or_null, const float* rgb_or_null,
                                   const void* zface_or_null, const float* verts, const int* faces, const float* vcolors3,
                                   const float* cams12_host, int n_frames, int H, int W, float tan_half_fov,
                                   float fov_range, double gathering_factor, unsigned seed, float ambient, int* counts2,
                                   float* cloud, float* cloud_rgb_or_null, long long* cloud_count, long long capacity,
                                   void* bins_store, float* zero6_or_null, float* zero1_or_null, int S, void* ws,
                                   size_t ws_bytes, void* stream);

/* line_segment_mesh_intersection (mu:120-151): hit[e] = 1 iff the ray from segs6[e][0:3] towards
 * segs6[e][3:6] meets a triangle at distance < |segment|. */
int nbp_segments_hit_mesh_f32(const float* verts, const int* faces, int n_faces, const float* segs6,
                              int n_segs, int* hit, void* stream);
/* check_camera_in_mesh (next_best_path/utility/long_term_utils.py:158-170): counts3[k] = number
 * of triangles hit from pts3[k] along +Y, +X, +Z (inside iff all three are odd). */
int nbp_axis_ray_counts_f32(const float* verts, const int* faces, int n_faces, const float* pts3,
                            int n_pts, int* counts3, void* stream);
/* GT obstacle label of a training record: get_binary_obstacle_array (next_best_path/utility/utils.py:226-262,
 * trimesh mesh_plane + matplotlib + PIL in the reference).  out [S,S] fp32 in {0,1}: 1 where the pixel centre is
 * within half_width_px of the intersection of the mesh with the plane y = y0; the window is [lo,hi] around
 * (cx, cz), column ~ -(x - cx), row ~ -(z - cz) (the reference's axes after its left-right flip).
 * The reference's line width is 1.5 pt at 100 dpi = 2.08 px: half_width_px = 1.04.  Parity unpinned
 * (third-party rasterisation); oracle/slice_raster.py restates THIS definition bit for bit. */
int nbp_slice_obstacle_f32(const float* verts, const int* faces, int n_faces, float y0, float cx, float cz,
                           int S, float lo, float hi, float half_width_px, float* out, void* stream);
/* The same label on the REFERENCE's pixel grid (round 6; pinned by tests/golden/obstacle_label.npz, which the reference's own
 * draw -> PNG -> resize -> threshold stage produced from this library's mesh / plane segments).  utils.py:232-258 draws into the
 * axes of a 2.56 in x 2.56 in figure at 100 dpi (default subplot box 198.4 x 197.12 px), x limits +-view/2 around the camera and
 * the y limits shrunk to keep the aspect (adjustable='datalim': 79.48 units for 80), saves the axes box ('tight' includes it:
 * 198 x 197 px), resizes to S x S and flips left-right.  So a world point lands on u = ((cx - x) + half_u) scale_u,
 * v = ((cz - z) + half_v) scale_v with scale_u = 2.48 * 256 / 198, scale_v = 2.48 * 256 / 197 px per unit at S = 256, and a
 * 1.5 pt stroke with projecting caps is half_width_px = cap_px = 1.347 px there (nextbestpath_amd/utility/hipops.py::
 * reference_figure_geometry).  cap_px = 0: round stroke ends, as nbp_slice_obstacle_f32.  What stays unpinned is Agg's
 * anti-aliasing and PIL's Lanczos filter themselves: the labels agree with the reference's to within one pixel of line position
 * (tests/test_training_data_cpu.py), not pixel for pixel. */
int nbp_slice_obstacle_fig_f32(const float* verts, const int* faces, int n_faces, float y0, float cx, float cz,
                               int S, float half_u, float scale_u, float half_v, float scale_v, float half_width_px,
                               float cap_px, float* out, void* stream);
/* nbp_slice_obstacle_fig_f32 for n <= 16 poses in one launch (training collection, round 7): item r has its own mesh (verts[r],
 * faces[r], n_faces[r]: HOST arrays of device pointers / counts) and y0_cx_cz_host[r][3]; the figure geometry is shared.  out
 * [n][S][S] (caller-owned, contiguous) is cleared once; bit-identical to n calls of nbp_slice_obstacle_fig_f32.  NBP_E_ARG for
 * n < 1, n > 16 or a missing / empty item. */
int nbp_slice_obstacle_fig_batch_f32(int n, const float* const* verts, const int* const* faces, const int* n_faces,
                                     const float* y0_cx_cz_host, int S, float half_u, float scale_u, float half_v, float scale_v,
                                     float half_width_px, float cap_px, float* out, void* stream);
/* Boltzmann goal scores of trajectory collection (next_best_path/utility/nbp_utils.py:695-745) for n <= 16 rollouts that replan,
 * one launch.  Item r: lattice positions pos3[r] [n_pos[r]][3] (device), the pose's (cx, cz) in cxcz_host[r][2], its value map
 * out1[r] [8][V][V] (device).  Per node p: cell[r][p] = row * V + col of the node's value-map cell in the pose's frame, -1 outside
 * the window (the in-window flag); val[r][p] = max over the 8 headings of out1 at the cell clamped into [0, V-1]^2.  Bit-identical
 * to transform_points_to_n_pieces + get_point_position_in_the_img + out1.amax(0)[clamp, clamp].  Outputs caller-owned. */
int nbp_goal_values_batch_f32(int n, const float* const* pos3, const int* n_pos, const float* cxcz_host, const float* const* out1,
                              int V, float lo, float hi, int* const* cell, float* const* val, void* stream);
/* Hindsight relabelling cells of trajectory collection (nbp_utils.py:655-693) for n <= 16 finished path segments, one launch.
 * Item r: the segment's poses xz[r] [m[r]][2] = (x, z) fp32 (device), 1 <= m[r] <= 4096.  cells[r] [m][m] int32 (caller-owned):
 * [i][j] = row * V + col of pose j in the frame of pose i for j > i when it lies in the value map's window, else -1.  Same fp32
 * operations as transform_points_to_n_pieces + get_point_position_in_the_img (rint, half to even). */
int nbp_hindsight_cells_batch_i32(int n, const float* const* xz, const int* m, int V, float lo, float hi, int* const* cells,
                                  void* stream);
/* Depth-map space carving of proxy points (A20): Camera.get_points_in_fov (mu:2849-2884) +
 * get_signed_distance_to_depth_maps (mu:2900-2949) + Scene.update_proxy_supervision_occ /
 * update_proxy_out_of_field (mu:3329-3363) fused per point.  For each proxy point inside the frustum
 * and closer than fov_range: sd = z_view - bilinear(depth) (invalid pixels = 1.1 zfar);
 * n_inside += 1; n_behind += (sd >= -tol); occ = (n_behind/n_inside >= score_threshold);
 * out_of_field = 0.  cam12 is a HOST array (one camera).  Not reachable from the NBP drivers. */
int nbp_carve_update_f32(const float* proxy_pts3, int P, const float* depth,
                         const unsigned char* mask_or_null, const float* cam12_host, int H, int W,
                         float tan_half_fov, float zfar, float fov_range, float tol,
                         float score_threshold, float* n_inside, float* n_behind, float* occ,
                         float* out_of_field, void* stream);
/* View-state vectors of the proxy points -- compute_view_state (macarons/utility/scone_utils.py:799-862) as
 * Scene.update_proxy_view_states applies it (macarons/utility/macarons_utils.py:3268-3327): for every selected point and every
 * camera position x_view_host [n_view <= 8][3] (HOST array), the direction point -> camera in spherical coordinates
 * (macarons/utility/CustomGeometry.py:27-45) is rounded to the nearest of n_elev x n_azim directions and
 * view_states[point][n_elev * n_azim] gets a 1.0 there (the reference's `+= ...; heaviside`, i.e. OR).  A point is selected
 * when mask_or_null[i] != 0 (NULL = all) and sd_or_null[i] < distance_to_surface (NULL = no such test).
 * nbp_carve_view_update_f32 = nbp_carve_update_f32 + that update for ONE camera at x_cam_host[3] in the same launch, over the
 * points inside the field of view with signed distance < distance_to_surface (macarons/testers/scene.py:598-607);
 * fov_mask_or_null [P] / sd_or_null [P] receive the field-of-view mask and the signed distances (sd only where the mask is 1). */
int nbp_view_state_update_f32(const float* pts3, int P, const unsigned char* mask_or_null, const float* sd_or_null,
                              float distance_to_surface, const float* x_view_host, int n_view, int n_elev, int n_azim,
                              float* view_states, void* stream);
/* Geometric coverage-gain model for candidate poses (stand-in for the unreleased SCONE predictor the reference calls at
 * macarons/testers/scene.py:640-670): gains[c] = number of proxy points inside candidate c's field of view (cams12_host [n][12],
 * range fov_range) with occ > 0.5 whose view-state bit for the direction towards x_cams_host[c] is still 0. */
int nbp_view_gain_i32(const float* pts3, int P, const float* occ, const float* view_states, const float* cams12_host,
                      const float* x_cams_host, int n_cams, int n_elev, int n_azim, int H, int W, float tan_half_fov,
                      float fov_range, int* gains, void* stream);
int nbp_carve_view_update_f32(const float* proxy_pts3, int P, const float* depth, const unsigned char* mask_or_null,
                              const float* cam12_host, int H, int W, float tan_half_fov, float zfar, float fov_range,
                              float tol, float score_threshold, float* n_inside, float* n_behind, float* occ,
                              float* out_of_field, const float* x_cam_host, int n_elev, int n_azim,
                              float distance_to_surface, float* view_states, unsigned char* fov_mask_or_null,
                              float* sd_or_null, void* stream);
/* ---- Scene / Cell point store (MACARONS scene objects, macarons/utility/macarons_utils.py:2952-3234), device resident.
 * store_pts [n_cells][capacity][3] fp32 + store_count [n_cells] int32, n_cells = grid3[0]*grid3[1]*grid3[2] in the
 * cartesian product order (i_l, i_w, i_h) of Scene.__init__ (:3063-3066); box6_host = x_min[3], x_max[3] of the scene.
 *
 * nbp_scene_fill_cells_f32 = Scene.fill_cells (:3177-3187) + Cell.fill (:3000-3028): points inside the scene box
 * (inclusive) go to the cell given by floor_divide (macarons/utility/utils.py:113-117) if they lie STRICTLY inside that
 * cell's box; a cell that receives more than n_point_min candidates drops those within `resolution` (fp64 distance,
 * d <= resolution) of a point it already stores -- new points are not compared with each other -- and appends the rest;
 * above `capacity` an exact-size seeded random subset of [stored | new] survives (torch.randperm(len)[:capacity], :3021).
 * n_dev_or_null (device int64) optionally bounds n on the device (cloud counters). */
size_t nbp_scene_fill_workspace_bytes(const float* box6_host, const int* grid3_host, int capacity,
                                      long long n_pts_max, double resolution);
int nbp_scene_fill_cells_f32(const float* pts3, long long n, const long long* n_dev_or_null,
                             const float* box6_host, const int* grid3_host, int capacity, double resolution,
                             int n_point_min, unsigned seed, float* store_pts, int* store_count, void* ws,
                             size_t ws_bytes, void* stream);
/* Scene.return_entire_pt_cloud (:3217-3234): the cells' points back to back, *n_out (device) = their number. */
int nbp_scene_gather_f32(const float* store_pts, const int* store_count, int n_cells, int capacity, float* out3,
                         long long out_capacity, long long* n_out, void* stream);
/* Scene.scene_coverage (:3512-3539): covered_and_total2[0] = number of stored GT points whose nearest recovered point
 * OF THE SAME CELL is closer than epsilon (fp64, strict), [1] = number of stored GT points; coverage = [0] / [1]. */
size_t nbp_scene_coverage_workspace_bytes(const float* box6_host, const int* grid3_host, int capacity_rec,
                                          double epsilon);
int nbp_scene_coverage_f32(const float* gt_pts, const int* gt_count, int capacity_gt, const float* rec_pts,
                           const int* rec_count, int capacity_rec, const float* box6_host, const int* grid3_host,
                           double epsilon, int* covered_and_total2, void* ws, size_t ws_bytes, void* stream);
/* Camera.get_points_in_fov (mu:2849-2884) for n_cams cameras (host [n_cams,12]): mask[cam][i] = 1 iff point i projects
 * inside the image, lies in front of the camera and closer than fov_range to its centre; any[cam] = 1 iff some point
 * does (Camera.is_fov_empty over the mesh vertices, mu:2672-2688).  Either output may be null. */
int nbp_points_in_fov_u8(const float* pts3, int P, const float* cams12_host, int n_cams, int H, int W,
                         float tan_half_fov, float fov_range, unsigned char* mask_or_null, int* any_or_null,
                         void* stream);
/* out3[j] = pc3[perm(j)], j < min(N, k): the first k points of a seeded random permutation of the cloud
 * (fill_surface_scene, mu:715-716); *m_out (device) = their number. */
int nbp_sample_points_f32(const float* pc3, long long N, const long long* N_dev_or_null, long long k, unsigned seed,
                          float* out3, long long* m_out, void* stream);
/* dst[offset + i] = pts3_host[i] for i < n <= 8 (the camera trajectory buffer, without a blocking copy). */
int nbp_append_points_f32(float* dst, long long offset, const float* pts3_host, int n, void* stream);
/* Host mirror of the sampling bijection (driver / tests). */
unsigned nbp_perm_index_host(unsigned j, unsigned n, unsigned seed);

/* ================================================================ A8-A12: planner
 * Obstacle fusion (next_best_path/testers/nbp_planning.py:166-191): obst = out2 >= threshold;
 * where the projection of the whole cloud (maps6 ch0..4 summed) is non-empty take (ch5 > 0);
 * zero where traj > 0.  fullproj = min(sum, 1)  (:172-175). */
int nbp_fuse_obstacle_f32(const float* out2, const float* maps6, const float* traj, float threshold,
                          int S, float* obst, float* fullproj, void* stream);
/* Candidate scoring (nbp_planning.py:203-231 + macarons_utils.py:86-100) for P lattice positions:
 * valid[i] iff the V-grid cell is inside and the 21x21 window of fullproj around the S-grid cell
 * contains a pixel == 1; cell2[i] = V-grid cell; score[i] = max_c out1[c,cell] - 10*fullproj[S cell]
 * in float64 (Python float arithmetic of the reference). */
int nbp_score_candidates_f32(const float* pos3, int P, float cx, float cz, const float* out1, int V,
                             const float* fullproj, int S, float lo, float hi,
                             const unsigned char* skip_or_null, unsigned char* valid, int* cell2,
                             double* score, void* stream);
/* line_across_image_pixel (long_term_utils.py:300-331) for E lattice edges in one launch:
 * blocked iff an endpoint maps outside the S x S image or >= 2 Bresenham pixels equal 1. */
int nbp_edges_blocked_u8(const float* obst, int S, float lo, float hi, float cx, float cz,
                         const float* pos3, const int* edges2, int E, unsigned char* blocked,
                         void* stream);
/* The three of them for the n <= 16 replanning rollouts of a lock-step group in two launches (fusion; scoring + edge mask):
 * HOST arrays of n entries (device pointers / scalars), poses_xz_host [n][2] = (cx, cz), skip entries may be NULL.
 * Identical results to the single calls. */
int nbp_replan_batch_f32(int n, const float* const* out2, const float* const* maps6, const float* const* traj, float threshold,
                         int S, float* const* obst, float* const* fullproj, const float* const* pos3, const int* P,
                         const float* poses_xz_host, const float* const* out1, int V, float lo, float hi,
                         const unsigned char* const* skip, unsigned char* const* valid, int* const* cell2,
                         double* const* score, const int* const* edges2, const int* E, unsigned char* const* blocked,
                         void* stream);
/* HOST function (no kernel, no stream): the candidate loop of nbp_planning.py:233-249 around
 * generate_Dijkstra_path (long_term_utils.py:334-418) on the position lattice, after the three kernels above
 * and their device->host copies.  Nodes 0..P-1 in lexicographic (i,j,k) order (idx3 [P,3], pos3 [P,3] world
 * positions); directed edges edges2 [E,2] grouped by source node in the reference's neighbour order
 * (+x,-x,+z,-z), edge_first [P+1] = first edge of each node.  An edge is usable iff pass_mask[q] or (not
 * blocked[q] and not coll_mask[q]) (ref :350-360); the search tree is the reference's uniform-cost tree (heap
 * ordered by (cost, tuple), came_from fixed at first discovery).  Candidates cand[] are tried in order (already
 * sorted by the caller: stable, score descending): path to the candidate, per node the best-valued heading of
 * out1 [8,V,V] at the node's value cell (cell = rint((-(p - c) - lo) * sc) in fp32) that hist5 [n_hist,5] does
 * not hold yet (ref :390-413), first node dropped (ref :416); when check_first_edge and the first edge crosses
 * the mesh (mesh_hit [E]) the pair is reported in new_coll2 (node ids a,b; the caller appends [a,b] and [b,a] to
 * its collision list) and the next candidate is tried on the rebuilt tree.  Outputs: *path_len = number of nodes
 * written to path_nodes / path_heads (0 = candidate is the start node; -1 = "None": the last candidate tried
 * was unreachable, or there was none); *goal = accepted candidate or -1.  *path_len = -2: a path node lies
 * outside the value map, where the reference draws a random heading -- the caller runs its own (Python) form of
 * this function so that the draw comes from the rollout's random stream; nothing was modified. */
int nbp_plan_search_host(int P, const int* idx3, const float* pos3, int E, const int* edges2,
                         const int* edge_first, const unsigned char* mesh_hit, const unsigned char* blocked,
                         const unsigned char* coll_mask, const unsigned char* pass_mask, const int* cand,
                         int n_cand, int start_id, float cx, float cz, const float* out1, int V, float lo,
                         float sc, const int* hist5, int n_hist, int check_first_edge, int max_path,
                         int* path_nodes, int* path_heads, int* path_len, int* goal, int* new_coll2,
                         int max_new_coll, int* n_new_coll);
/* calculate_coverage_percentage (long_term_utils.py:437-468): *count_out = #{g : min_j |gt_g - s_j|
 * < threshold} where s = the cloud, or a seeded random subset of sample_k points of it when it
 * has more (random_sample_pc, :437-447); *m_out = number of points used.  bbox_* = bounds of gt. */
size_t nbp_coverage_workspace_bytes(const float* bbox_lo_host, const float* bbox_hi_host,
                                    float threshold, long long sample_k);
int nbp_coverage_count_f32(const float* gt3, int G, const float* pc3, long long N,
                           const long long* N_dev_or_null, long long sample_k, unsigned seed,
                           float threshold, const float* bbox_lo_host, const float* bbox_hi_host,
                           int* count_out, int* m_out, void* ws, size_t ws_bytes, void* stream);
/* The same count when the GT cloud is reused over many calls (one rollout): nbp_coverage_plan_build_f32 sorts gt into a
 * grid once (plan = caller-owned device buffer of nbp_coverage_plan_bytes); nbp_coverage_count_planned_f32 then runs one
 * kernel over the sampled cloud points.  It ADDS to *count_accum (caller zeroes it) and needs an `epoch` > 0 that differs
 * between consecutive calls on the same plan (per-GT-point stamps instead of a clear). */
size_t nbp_coverage_plan_bytes(const float* bbox_lo_host, const float* bbox_hi_host, float threshold, int G);
size_t nbp_coverage_plan_workspace_bytes(const float* bbox_lo_host, const float* bbox_hi_host, float threshold, int G);
int nbp_coverage_plan_build_f32(const float* gt3, int G, float threshold, const float* bbox_lo_host,
                                const float* bbox_hi_host, void* plan, size_t plan_bytes, void* ws,
                                size_t ws_bytes, void* stream);
int nbp_coverage_count_planned_f32(void* plan, int G, float threshold, const float* bbox_lo_host,
                                   const float* bbox_hi_host, const float* pc3, long long N,
                                   const long long* N_dev_or_null, long long sample_k, unsigned seed,
                                   unsigned epoch, int* count_accum, int* m_out, void* stream);

/* ================================================================ A2-A3: training step
 * Kernels behind the autograd functions of nextbestpath_amd/networks/training.py, which replace
 * autograd + cuDNN under train_experience_data (next_best_path/utility/nbp_utils.py:340-395) for
 * the layers of next_best_path/networks/nbp_model.py:8-62 in nbp.train() mode.  All [M, C] tensors
 * are NHWC with M = B*H*W.  Reductions are two-stage => deterministic. */
size_t nbp_colreduce_workspace_bytes(long long M, int C);
/* nn.BatchNorm2d training forward (eps, momentum = module values): batch mean / biased variance,
 * running-stat update (unbiased variance; pass NULL to skip), y = [relu]((x-mean)*invstd*gamma+beta);
 * mean / invstd are saved for the backward. */
int nbp_bn_train_forward_f32(const float* x, long long M, int C, const float* gamma, const float* beta,
                             float eps, float momentum, float* running_mean, float* running_var,
                             int relu, float* mean, float* invstd, float* y, void* ws, size_t ws_bytes,
                             void* stream);
/* Backward of the above (+ fused ReLU mask from y when relu != 0): dx, dgamma, dbeta. */
int nbp_bn_train_backward_f32(const float* dy, const float* x, const float* y_or_null, long long M, int C,
                              const float* mean, const float* invstd, const float* gamma, int relu,
                              float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                              void* stream);
/* The same two with their consumers' passes folded in (C % 4 == 0; nbp_bn_backward_fuses(C) tells): the forward also writes
 * max |y| into amax_out (64 zeroed words, float bits by atomicMax: the operand scale of the split convolution that reads y); the
 * backward also writes dx_colsum[c] = sum_m dx[m][c] (the bias gradient of the convolution in front of this BatchNorm) and
 * max |dx| into amax_out (the scale of that convolution's data / weight gradients) -- in the pass that writes dx, instead of
 * two more reads of it.  NULL outputs are skipped. */
int nbp_bn_train_forward_amax_f32(const float* x, long long M, int C, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var,
                                  int relu, float* mean, float* invstd, float* y, void* amax_out, void* ws,
                                  size_t ws_bytes, void* stream);
int nbp_bn_backward_fuses(int C);
int nbp_bn_train_backward_fused_f32(const float* dy, const float* x, const float* y_or_null, long long M, int C,
                                    const float* mean, const float* invstd, const float* gamma, int relu,
                                    float* dx, float* dgamma, float* dbeta, float* dx_colsum, void* amax_out,
                                    void* ws, size_t ws_bytes, void* stream);
/* Round 4: the backward without reading y.  nbp_bn_train_forward_stat4_f32 = nbp_bn_train_forward_amax_f32 that also hands out the
 * UNROUNDED statistics the normalisation used (stat_out: [4 C] doubles, 32-byte aligned: mean | invstd | lo | hi, the last two with
 * relu only: y > 0 <=> lo <= x <= hi exactly, two floats per channel found by bisection with the forward's own arithmetic);
 * nbp_bn_train_backward_stat_f32 = nbp_bn_train_backward_fused_f32 whose ReLU mask (y > 0) is rebuilt from x -- which the pass
 * reads anyway -- through the forward's own arithmetic on those statistics (C % 4 == 0): two tensor reads less per BatchNorm and
 * step, the same mask bit for bit. */
/* (round 6: `stat_doubles` = the doubles behind stat_out, NBP_E_WS below 4 C; without relu the two bounds are written as
 * (-inf, +inf).  The names changed with the signature -- ..._stat_f32 / ..._part_f32 of rounds 4-5 are gone -- so a caller built for the
 * [2 C] contract of round 4 fails to link instead of being overrun.) */
int nbp_bn_train_forward_stat4_f32(const float* x, long long M, int C, const float* gamma, const float* beta,
                                   float eps, float momentum, float* running_mean, float* running_var,
                                   int relu, float* mean, float* invstd, float* y, void* amax_out, double* stat_out, int stat_doubles,
                                   void* ws, size_t ws_bytes, void* stream);
int nbp_bn_train_backward_stat_f32(const float* dy, const float* x, const double* stat_d, const float* beta, long long M, int C,
                                   const float* mean, const float* invstd, const float* gamma, int relu,
                                   float* dx, float* dgamma, float* dbeta, float* dx_colsum, void* amax_out,
                                   void* ws, size_t ws_bytes, void* stream);
/* out[c] = sum_m rows[m]*x[m][c] (rows NULL = 1): conv bias gradients, psi weight gradient. */
int nbp_colsum_f32(const float* x, const float* rows_or_null, long long M, int C, float* out, void* ws,
                   size_t ws_bytes, void* stream);
/* op 0: relu(a+b)  1: a*(b>0)  2: sigmoid(a)  3: a*b*(1-b)  4: a+b  5: a+b[0] */
int nbp_elementwise_f32(int op, const float* a, const float* b, long long n, float* out, void* stream);
/* out[m][c] = sum_k src_k[m ld_k + c] (k = 0 .. n - 1, left to right in fp32; n <= 8; C % 4 == 0; 16-byte aligned pointers; ld_k >= C
 * floats, a multiple of 4: a source may be a channel slice of a wider NHWC tensor).  The gradient of an activation with n consumers
 * (a skip connection: max-pool + two attention gates x two uses) in one pass instead of autograd's n - 1 binary adds -- what
 * loss.backward() does implicitly in next_best_path/utility/nbp_utils.py:383.  srcs_host / ld_host: HOST arrays of n entries. */
int nbp_sum_n_f32(int n, const float* const* srcs_host, const long long* ld_host, long long M, int C, float* out, void* stream);
/* The element-wise middle of Attention_block in TRAINING mode (nbp_model.py:52-60), between the two 1x1 convolutions and x * psi:
 *     g1 = BN_g(g_pre);  x1 = BN_x(x_pre);  q = relu(g1 + x1);  p = q . w_psi + b_psi        (batch statistics, running stats updated)
 * fused: two statistics passes + ONE pass that reads g_pre / x_pre and writes q [M,F] and p [M] (the separate launches were BatchNorm
 * apply twice, add-relu and a row-dot: 8 tensor passes for 3), and its backward from dp = dL/dp: both BatchNorm backwards, the ReLU
 * mask, dq = dp (x) w_psi and the psi weight's gradient in one reduce + one apply pass (15 tensor passes for 8).  Every output is the
 * separate launches' bit for bit (p sums its row in nbp_rowdot_f32's order).  F = F_int: F / 4 a power of two in [4, 64].  stat_g / stat_x: [4 F] doubles, 32-byte aligned; csum_* = column sums of d g_pre / d x_pre (the 1x1 convolutions' bias
 * gradients), amax_* (or NULL) = 64 zeroed words receiving max |.| of them; ws >= nbp_gate_mid_workspace_bytes(M, F). */
size_t nbp_gate_mid_workspace_bytes(long long M, int F);
int nbp_gate_mid_forward_f32(const float* g_pre, const float* x_pre, long long M, int F,
                             const float* gamma_g, const float* beta_g, float* run_mean_g, float* run_var_g, float eps_g, float mom_g,
                             const float* gamma_x, const float* beta_x, float* run_mean_x, float* run_var_x, float eps_x, float mom_x,
                             float* mean_g, float* invstd_g, float* mean_x, float* invstd_x, double* stat_g, double* stat_x,
                             const float* w_psi, const float* b_psi, float* q, float* p, void* ws, size_t ws_bytes, void* stream);
int nbp_gate_mid_backward_f32(const float* dp, const float* w_psi, const float* q, const float* g_pre, const float* x_pre,
                              long long M, int F, const float* mean_g, const float* invstd_g, const float* gamma_g,
                              const float* mean_x, const float* invstd_x, const float* gamma_x, float* dg_pre, float* dx_pre,
                              float* dgamma_g, float* dbeta_g, float* dgamma_x, float* dbeta_x, float* dw_psi, float* csum_g,
                              float* csum_x, void* amax_g, void* amax_x, void* ws, size_t ws_bytes, void* stream);
int nbp_rowscale_f32(const float* x, const float* s, long long M, int C, float* out, void* stream);
/* ... that also leaves max |out| in the 64 zeroed words of amax_out (C % 4 == 0, 16-byte aligned tensors, else NBP_E_SHAPE). */
int nbp_rowscale_amax_f32(const float* x, const float* s, long long M, int C, float* out, void* amax_out, void* stream);   /* x[m][c]*s[m] */
/* backward of out = x * s[m] in one pass: dx[m][c] = dy[m][c] * s[m], ds[m] = sum_c dy[m][c] * x[m][c]; dy's rows are ldy >= C floats
 * apart (a channel slice of a wider gradient is read in place); C, ldy multiples of 4, 16-byte aligned pointers (else NBP_E_SHAPE) */
int nbp_rowscale_backward_f32(const float* dy, long long ldy, const float* x, const float* s, long long M, int C, float* dx,
                              float* ds, void* stream);
int nbp_rowdot_f32(const float* a, const float* b, int b_is_vector, long long M, int C, float* out,
                   void* stream);                                                                     /* sum_c a*b   */
int nbp_outer_f32(const float* s, const float* w, long long M, int C, float* out, void* stream);      /* s[m]*w[c]   */
/* nn.MaxPool2d(2,2) backward (gradient to the first maximum of each window, ATen rule). */
int nbp_maxpool2_backward_f32(const float* x, const float* dy, int B, int H, int W, int C, float* dx,
                              void* stream);
/* nn.Upsample(x2, nearest) backward: 2x2 block sums, dy [B,2Hs,2Ws,C] -> [B,Hs,Ws,C]. */
int nbp_sum2x2_f32(const float* dy, int B, int Hs, int Ws, int C, float* out, void* stream);
int nbp_slice_channels_f32(const float* in, long long M, int Cin, int c0, int Cs, float* out, void* stream);
int nbp_pad_channels_f32(const float* in, long long M, int Cin, int Cout, float* out, void* stream);
/* Forward packing with zero padding of both channel counts: dst[ci/32][tap][Npad][32]. */
int nbp_pack_conv_weight_padded(const float* w_oihw, int N, int C, int ksize, int Cpad, int Npad, float* dst,
                                void* stream);
/* Data gradient = nbp_conv_igemm_f32 on dY with these weights: flipped taps, co <-> ci transposed,
 * zero padded to (Cpad, Npad) multiples of 32: dst[co/32][tap][ci][co%32]. */
int nbp_pack_conv_weight_dgrad(const float* w_oihw, int N, int C, int ksize, int Cpad, int Npad, float* dst,
                               void* stream);
/* Weight gradient on the matrix cores: dW [n_real][c_real][k][k] (OIHW) of
 * out = conv(cat(src0, src1) [x2 upsampled]) given dY [B,H,W,N]; C0, C1, N multiples of 64. */
size_t nbp_conv_wgrad_workspace_bytes(int B, int H, int W, int C0, int C1, int N, int ksize);
int nbp_conv_wgrad_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                       int ksize, const float* dy, int N, int c_real, int n_real, float* dw, void* ws,
                       size_t ws_bytes, void* stream);
/* nbp_conv_wgrad_f32 with the products of the 3x3 layers on the fp16 matrix pipe: every fp32 operand (X, dY) scaled by a
 * power of two from its tensor's max |.| (computed inside), cut into two fp16 pieces, three exact MFMAs per product, fp32
 * accumulation (the scheme of nbp_conv3x3_split_f32; error vs fp64 <= the fp32 MFMA pipe's).  amax*_or_null: 64-word max-|.|
 * slots (nbp_amax_f32) of src0 / src1 / dy when the caller has them (any upper bound of the tensor's max works: e.g. the forward's
 * joint slot for both sources), else taken inside.  Same other arguments and workspace; layers the split kernel does not take (1x1, W % 32 != 0) run nbp_conv_wgrad_f32. */
int nbp_conv_wgrad_split_f32(const float* src0, int C0, const float* src1, int C1, int ups, int B, int H, int W,
                             int ksize, const float* dy, int N, int c_real, int n_real, float* dw,
                             const void* amax0_or_null, const void* amax1_or_null, const void* amaxy_or_null, void* ws,
                             size_t ws_bytes, void* stream);
/* Sparse value targets (nbp_utils.py:373-379): pred[k] = out1[b,c,x,y], coords [K,4] int64; and the
 * scatter-add of its gradient into a zeroed d_out1. */
int nbp_gather_values_f32(const float* out1_nchw, const long long* coords_bcxy, int K, int C, int H, int W,
                          float* pred, void* stream);
int nbp_scatter_values_f32(const float* dpred, const long long* coords_bcxy, int K, int C, int H, int W,
                           float* dout1_nchw_zeroed, void* stream);
/* mode 0: sum (p-t)^2, mode 1: sum BCE(p,t) (log clamped at -100 like torch) into *sum_out (device
 * double); dp (optional) = grad_coef * d(mean loss)/dp. */
int nbp_loss_f32(int mode, const float* p, const float* t, long long n, float grad_coef, double* sum_out,
                 float* dp_or_null, void* ws, size_t ws_bytes, void* stream);
/* Exact D4 symmetry augmentation of a training batch (csrc/nbp_augment.hip).  The reference defines augment_data
 * (next_best_path/utility/nbp_utils.py:267-289: flips and 90-degree rotations of the images, p = 0.4) and never calls it; as
 * written it turns only the images (the sparse targets stay where they were) and an array flip i -> S-1-i moves the input by one
 * pixel but the value map by one cell.  Here the planes move about the CAMERA: pixel index i = rint((v + 40) S / 80) puts the camera
 * at S/2, so the reflection v -> -v is i -> S - i.  ops_dev: B op codes on the device, bit 0 = transpose (rows <-> cols), bit 1 =
 * reflect rows, bit 2 = reflect cols, applied in that order:
 *     transpose     out[r][c] = in[c][r]
 *     reflect rows  out[r][c] = in[S - r][c] for r >= 1, out[0][c] = 0 (the mirror image of index 0 is index S, outside the array)
 * x [B,5,S,S] and gt [B,1,S,S] NCHW fp32 -> x_out, gt_out (out of place, nothing may alias), all 6 B planes in one launch; bit-exact
 * moves.  The targets' cells and heading channels are remapped on the host (utility/augment.py).  NBP_E_ARG: null pointer, B < 1,
 * aliasing buffers; NBP_E_SHAPE: S % 16 != 0, 6 B > 65535, a pointer off the 16-byte grid; nothing is written on an error. */
int nbp_augment_batch_f32(const float* x, const float* gt, const int* ops_dev, int B, int S, float* x_out, float* gt_out,
                          void* stream);
/* The D4 symmetry ensemble of the eval forward (csrc/nbp_ensemble.hip; not in the reference): the network is run on n
 * moved copies of every input and the outputs, moved back, are averaged.  ops_dev: n op codes (as above) on the device, 1 <= n <= 8.
 *   expand   x [B,5,S,S] -> x_out [n,B,5,S,S], x_out[k][b] = ops[k] applied to x[b]; bit-exact moves, one launch.
 *   reduce   raw1 [n,B,8,S/4,S/4], raw2 [n,B,1,S,S] (the outputs on the expanded batch) -> out1 [B,8,S/4,S/4], out2 [B,1,S,S]:
 *            member k is moved back by the inverse element of ops[k] (itself, except that codes 3 and 5 swap); a value map's heading
 *            channels are permuted with it (utility/augment.py::transform_value_map).  The moved members are summed in fp32 in the
 *            order k = 0 .. n-1 and each cell is divided by the number of members that reach it: a member whose inverse reflects
 *            rows does not reach row 0, likewise columns (utility/augment.py::ensemble_reference is the float64 definition).  One
 *            launch, no atomics: two runs give the same bits.
 * Out of place, nothing may alias.  NBP_E_ARG: null pointer, B < 1, n outside 1..8, aliasing buffers; NBP_E_SHAPE: S % 16 != 0, more
 * than 65535 planes (5 n B / 9 B), a pointer off the 16-byte grid; nothing is written on an error. */
int nbp_ensemble_expand_f32(const float* x, int B, int S, const int* ops_dev, int n, float* x_out, void* stream);
int nbp_ensemble_reduce_f32(const float* raw1, const float* raw2, int B, int S, const int* ops_dev, int n, float* out1, float* out2,
                            void* stream);

/* The compact replay record (csrc/nbp_replay.hip; not in the reference): a lossless, bit-exact encoding of the 6
 * planes of a replay record ('current_model_input' [1,5,S,S] + 'current_gt_2d_layout' [1,1,S,S], fp32) whose definition is
 * nextbestpath_amd/utility/replay_codec.py ("NBPC" version 1): a 64-byte header, then per channel a bitmap of the pixels whose
 * fp32 bit pattern is not zero and those pixels at 0 (all 1.0f), 1 (u8), 2 (u16) or 4 (raw fp32 bits) bytes each.
 *   nbp_replay_stream_bound  the largest stream of a record of side S, 64 + 6 (S^2/8 + 4 S^2); 0 for an unsupported S.
 *   encode   rec [n,6,S,S] -> the stream of record r at arena + r * stride_bytes, byte for byte replay_codec.encode's, padding
 *            included; no byte of a slot beyond the stream's total_bytes is written.  stride_bytes >= nbp_replay_stream_bound(S)
 *            and a multiple of 16 (else NBP_E_WS).  Two launches, no atomics: two runs give the same bytes.
 *   decode   `streams`: one device byte buffer that holds n streams at the 16-byte-aligned byte offsets offsets_host[r] (a HOST
 *            array, read during the call: the offsets ride in the kernel arguments, 64 records per launch) -> x_out [n,5,S,S] and
 *            gt_out [n,1,S,S], every pixel written, zeros included.  The host validates the headers first
 *            (replay_codec.parse_header); the kernel clamps nnz, the widths and every value index again, so whatever the bytes it
 *            reads no further than nbp_replay_stream_bound(S) bytes behind an offset and writes nothing outside the outputs.
 * 16 <= S <= 512, S % 16 == 0, 16-byte aligned pointers (else NBP_E_SHAPE); NBP_E_ARG: null pointer, n < 1, an offset that is
 * negative or off the 16-byte grid; nothing is launched or written on an error. */
size_t nbp_replay_stream_bound(int S);
int nbp_replay_encode_f32(const float* rec, int n, int S, void* arena, size_t stride_bytes, void* stream);
int nbp_replay_decode_f32(const void* streams, const long long* offsets_host, int n, int S, float* x_out, float* gt_out,
                          void* stream);

/* Planner-facing validation metrics of one batch, per sample (csrc/nbp_metrics.hip; not in the reference; the
 * definition of record is nextbestpath_amd/utility/metrics.py).  out1 [B,8,S/4,S/4], out2 and gt [B,1,S,S] fp32; coords [K,3] int64
 * (heading, row, col), gains [K] fp32, bidx [K] int64 in any order (an index outside [0,B) belongs to no sample); thresholds_host: T
 * floats on the HOST, 1 <= T <= 8, read during the call (they ride in the kernel arguments).  Into caller memory:
 *   obst  int64 [B,T,4]  (tp, fp, fn, tn) of `out2 >= threshold` (fp32; a NaN is negative) against `gt > 0.5`
 *   rank  int64 [B,6]    (n, n_bad, comparable, concordant, discordant, hit) over the sample's targets in record order; a target
 *                        whose heading is outside [0,8) or whose row / column is outside [0,S/4) is counted in n_bad and never
 *                        dereferenced
 *   val   double [B,4]   (sum |p - g|, sum (p - g)^2, max g, g[pred_best]) over the good targets, in float64; zeros when n = 0
 * One memset of obst and two launches on `stream`, no host synchronisation, no allocation.  Integer atomics only, the float64 sums by
 * a fixed tree: two runs give the same bits.  K = 0 is legal (coords, gains and bidx may then be NULL).  NBP_E_ARG: null pointer,
 * B < 1, K < 0, T outside 1..8; NBP_E_SHAPE: S % 4 != 0, S outside 4..16384, B > 65535, out2 or gt off the 16-byte grid, an output off
 * the 8-byte grid; nothing is launched or written on an error. */
int nbp_val_metrics_f32(const float* out1, const float* out2, const float* gt, const long long* coords, const float* gains,
                        const long long* bidx, int B, int S, int K, int T, const float* thresholds_host, long long* obst,
                        long long* rank, double* val, void* stream);

/* ---- The optimizer step (csrc/nbp_optim.hip): the reference's torch.optim.AdamW(lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight decay
 * 0.01) of next_best_path/utility/nbp_utils.py:228 and its scaler.step(optimizer) / scaler.update() of nbp_utils.py:386-388 (a
 * GradScaler drops a step whose gradients hold an inf or a NaN), plus the global-norm clipping of torch.nn.utils.clip_grad_norm_,
 * as multi-tensor kernels over separately allocated fp32 tensors.  Host binding: nextbestpath_amd/optim.py::HipAdamW.
 * Tables on the device, built by the caller:
 *   descs   one record per tensor  { float* p; const float* g; float* m; float* v; int64 numel; }     (nbp_optim_desc_bytes() = 40)
 *   chunks  one record per workgroup { int64 first; int32 tensor; int32 pad; } (16 bytes): elements [first, first + chunk) of that
 *           tensor, clipped to numel; first is a multiple of nbp_optim_chunk_elems() (16384).  Any numel >= 1; 16-byte accesses
 *           where the tensor's four base addresses are 16-byte aligned, 4-byte accesses otherwise (the backward: same bits; the forward: the same terms, added in another order).
 *   state   nbp_optim_state_bytes(n_groups) = 32 + 8 n_groups bytes, zeroed before the first step:
 *           { f32 total_norm; f32 clip_coef; i32 finite; i32 applied; f32 step; i32 skipped_steps; i32 pad[2];
 *             { f32 bc1 = 1 - beta1^step; f32 sqrt_bc2 = sqrt(1 - beta2^step); } per param group }
 * nbp_optim_workspace_bytes(n_chunks): one double per chunk.  n_groups <= 16. */
int nbp_optim_desc_bytes(void);
int nbp_optim_chunk_elems(void);
size_t nbp_optim_workspace_bytes(long long n_chunks);
size_t nbp_optim_state_bytes(int n_groups);
/* clip_grad_norm_'s reduction (the norm behind nbp_utils.py:386-388's inf / NaN test): ws[c] = sum of g^2 over chunk c, products and
 * additions in double in an order fixed by element position (no atomics: two runs give the same bits). */
int nbp_grad_sqnorm_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, void* ws, size_t ws_bytes, void* stream);
/* One workgroup: total_norm = sqrt(sum of ws[0 .. n_chunks) in a fixed order, double); clip_coef = min(1, max_norm / (total_norm + 1e-6))
 * (clip_grad_norm_'s rule; exactly 1.0f when max_norm <= 0 = clipping off); finite = the sum is finite; the step is applied unless
 * skip_nonfinite and not finite (scaler.step, nbp_utils.py:386): then step += 1, the bias corrections of every group are recomputed
 * in double from betas_host [n_groups][2] (read during the call) and steps_or_null [n_steps] (the per-parameter `step` scalars of the
 * optimizer state, nbp_utils.py:228) all receive the new step; otherwise skipped_steps += 1 and nothing else moves.
 * ws_or_null = NULL: no norm pass ran (then max_norm <= 0 and skip_nonfinite = 0, else NBP_E_ARG): total_norm = 0, coef = 1. */
int nbp_optim_finalize_f32(const void* ws_or_null, int n_chunks, double max_norm, int skip_nonfinite, const double* betas_host,
                           int n_groups, void* state, void* steps_or_null, int n_steps, void* stream);
/* torch.optim.AdamW's update (nbp_utils.py:228) of the tensors the chunks name, for param group `group` of the state block:
 *   g^ = clip_coef g;  p <- p (1 - lr wd);  m <- beta1 m + (1 - beta1) g^;  v <- beta2 v + (1 - beta2) g^^2;
 *   p <- p - (lr / bc1) m / (sqrt(v) / sqrt_bc2 + eps)
 * m and v are evaluated in double and rounded once, p in fp32.  g is only read (clip_grad_norm_ scales the gradients in place; here
 * the coefficient is applied on load).  Writes nothing when the state block says the step is skipped (state.applied = 0). */
int nbp_adamw_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, const void* state, int group, double lr, double beta1,
                  double beta2, double eps, double weight_decay, void* stream);

/* ---- Weight averaging (csrc/nbp_ema.hip).  Not in the reference: an exponential moving average of the tensors of the
 * network under training, kept on the device behind the optimizer step.  Host binding: nextbestpath_amd/optim.py::WeightEMA.
 * Tables on the device, built by the caller:
 *   descs   one record per tensor  { const float* p; float* e; int64 numel; }                           (nbp_ema_desc_bytes() = 24)
 *   chunks  the optimizer's chunk records { int64 first; int32 tensor; int32 pad; }: nbp_optim_chunk_elems() elements of a tensor
 *           per workgroup.  Any numel >= 1; 16-byte accesses where p and e are 16-byte aligned, 4-byte accesses otherwise (same
 *           results).  p and e must not overlap.
 *   state   nbp_ema_state_bytes() = 16 bytes, zeroed before the first update: { i32 num_updates; i32 pad[3]; }
 * One update:  d = warmup ? min(decay, (1 + num_updates) / (10 + num_updates)) : decay   (double, on the device);
 *              e <- fl32(d e + (1 - d) p)   evaluated in double and rounded once;   num_updates += 1 (a one-thread launch behind the
 *              update's, so the workgroups that read the counter never race its increment).
 * optim_state_or_null: the state block of nbp_optim_finalize_f32, read behind it on the same stream; when its `applied` word is 0
 * (a step dropped for non-finite gradients) the update writes nothing: e and num_updates keep their bits.  NULL: always applied.
 * No atomics: two runs give the same bits.  NBP_E_ARG: null table or state, n_chunks < 1, decay outside [0, 1). */
int nbp_ema_desc_bytes(void);
size_t nbp_ema_state_bytes(void);
int nbp_ema_update_f32(const void* descs_dev, const void* chunks_dev, int n_chunks, void* ema_state, const void* optim_state_or_null,
                       double decay, int warmup, void* stream);

/* ---- The training objective with per-sample terms (csrc/nbp_objective.hip).  Not in the reference: what
 * loss-prioritised replay needs, and the fused form of gather + MSE + BCE (nbp_model.py:162-173, nbp_utils.py:373-381).  The
 * definition of record is nextbestpath_amd/utility/priority.py::objective_reference.  Host binding: hipops.objective_forward /
 * objective_backward, networks/training.py::ObjectiveFn.
 *   out1_nchw [B,C,H,W] fp32; coords_bcxy [K,4] int64 (b, c, x, y), rows in any order; gains [K] fp32; out2, gt [B,S,S] fp32;
 *   weights_or_null [B] fp32 (NULL: every weight 1).  A row with a coordinate out of range (b among them) contributes nothing.
 *   v_b = sum_{k: b_k = b} (out1[b,c,x,y] - gain_k)^2,  n_b = the number of those rows,
 *   o_b = sum_pixels -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))      (terms in fp32 as nbp_loss_f32 forms them, sums in double)
 * forward:  per_sample [B,3] double = (v_b, n_b, o_b);  totals [2] double = (sum_b w_b v_b, sum_b w_b o_b).  Two launches; every sum
 *           in a fixed order that depends on the sample's own data and S only (not on B, the slot b, or the position of its rows among
 *           the others'); no floating-point atomics: two runs give the same bits.  K = 0 is legal (v = n = 0).
 * backward: coef_dev [2] fp32 ON THE DEVICE = (dL/dmse, dL/dbce) for mse = totals[0] / K, bce = totals[1] / (B S^2);
 *           d_out2 [B,S,S] = coef1 w_b (p - t) / max(p (1 - p), 1e-12) / (B S^2);  d_out1 [B,C,H,W] zero-filled, then
 *           += coef0 w_b 2 (pred - gain) / K per row (atomicAdd: a cell named twice receives both).  One asynchronous fill and one
 *           launch, no host synchronisation.
 * ws: nbp_objective_workspace_bytes(B, S) bytes (0 for B < 1 or S < 1).  16-byte accesses where S^2 % 4 == 0 and out2 / gt / d_out2
 * are 16-byte aligned, 4-byte accesses otherwise (the backward: same bits; the forward: the same terms, added in another order).  NBP_E_ARG: a null pointer (coords / gains only when K > 0), B < 1,
 * S < 1, K < 0, C / H / W < 1; NBP_E_SHAPE: B > 65535 or S > 32768; NBP_E_WS: ws_bytes too small.  Nothing is written on an error. */
size_t nbp_objective_workspace_bytes(int B, int S);
int nbp_objective_forward_f32(const float* out1_nchw, const long long* coords_bcxy, const float* gains, int K, int C, int H, int W,
                              const float* out2, const float* gt, int B, int S, const float* weights_or_null, double* per_sample,
                              double* totals, void* ws, size_t ws_bytes, void* stream);
int nbp_objective_backward_f32(const float* out1_nchw, const long long* coords_bcxy, const float* gains, int K, int C, int H, int W,
                               const float* out2, const float* gt, int B, int S, const float* weights_or_null, const float* coef_dev,
                               float* d_out1_nchw, float* d_out2, void* ws, size_t ws_bytes, void* stream);

/* ---- Reconstruction-quality metrics (csrc/nbp_recon.hip).  Not in the reference: accuracy, completeness, Chamfer
 * distance and precision / recall / F-score of a rollout's cloud against the GT surface.  The definition of record is
 * nextbestpath_amd/utility/recon_metrics.py.  Host binding: hipops.nn_dist2 / recon_stats / ReconMetrics.
 *
 * Truncated exact nearest-neighbour squared distance, fp32:
 *   d2[i] = min(cap2, min over the targets j INSIDE THE BOX of ((ex ex + ey ey) + ez ez)),  e = t_j - q_i,  cap2 = fl(cap cap),
 * every operation rounded to fp32 (no contraction).  Inside the box: lo <= t <= hi on the three axes, compared in fp32 (a NaN is
 * outside); the caller chooses the box so that ignoring the others is harmless (the GT bounds grown by cap).  q3 [Q][3], t3 [T][3],
 * d2 [Q]; Q and T are host bounds and, where the *_dev_or_null pointer is given, the device counter (clipped to the bound) is the
 * length: rows at or beyond it are never read, entries of d2 at or beyond it are never written.  lo_host / hi_host [3]; hi == lo on
 * an axis is one cell.  cell = the width w > 0 of the uniform grid the in-box targets are counting-sorted into (cells of 1.001 w);
 * the query walks the shells of cells at Chebyshev distance r = 0 .. ceil(cap / w) around its cell and stops after shell r once
 * best <= fl(r w)^2: the result is the brute-force minimum bit for bit, and two runs give the same bits (no atomics on the output).
 * A query more than ceil(cap / w) cells outside the grid gets cap2 without a memory access.  Q = 0 and T = 0 are legal.
 *   nbp_nn_dist2_f32             sorts the targets and queries them (ws: nbp_nn_dist2_workspace_bytes)
 *   nbp_nn_plan_build_f32        sorts a static target set once into `plan` (nbp_nn_plan_bytes; ws: nbp_nn_plan_workspace_bytes)
 *   nbp_nn_dist2_planned_f32     queries a plan built with the same lo / hi / cell
 * No allocation, no host synchronisation.  NBP_E_ARG: a null pointer, a negative or > 2^31 - 1 count, cell or cap not positive and
 * finite, cap / cell > 2^24, hi < lo; NBP_E_SHAPE: more than 2048 cells on an axis (beyond that the fp32 cell coordinates no longer
 * carry the early exit's proof) or more than 2^28 cells; NBP_E_WS.  The size queries return 0 where the call would fail. */
size_t nbp_nn_plan_bytes(const float* lo_host, const float* hi_host, float cell, long long T);
size_t nbp_nn_plan_workspace_bytes(const float* lo_host, const float* hi_host, float cell, long long T);
int nbp_nn_plan_build_f32(const float* t3, long long T, const long long* T_dev_or_null, const float* lo_host, const float* hi_host,
                          float cell, void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, void* stream);
int nbp_nn_dist2_planned_f32(const void* plan, const float* lo_host, const float* hi_host, float cell, float cap, const float* q3,
                             long long Q, const long long* Q_dev_or_null, float* d2, void* stream);
size_t nbp_nn_dist2_workspace_bytes(const float* lo_host, const float* hi_host, float cell, long long T);
int nbp_nn_dist2_f32(const float* q3, long long Q, const long long* Q_dev_or_null, const float* t3, long long T,
                     const long long* T_dev_or_null, const float* lo_host, const float* hi_host, float cap, float cell, float* d2,
                     void* ws, size_t ws_bytes, void* stream);
/* Summary of d2 [n] (n: host bound, and the device counter where given): sums2 [2] float64 = (sum sqrt(d2), sum d2), the square root
 * taken in float64; counts [T] int64 = #{ sqrtf(d2) < thresholds_host[t] }, decided as d2 <= the largest float whose sqrtf is below
 * the threshold (the same decision: sqrtf is monotone and correctly rounded).  1 <= T <= 8 thresholds on the HOST, positive and
 * finite.  Two launches of a fixed geometry: per-thread strided float64 partials, a fixed tree inside the block, one stored row
 * per block, the rows added in index order -- no floating-point atomics, two runs give the same bits.  n = 0 gives zeros.
 * ws: nbp_recon_stats_workspace_bytes().  NBP_E_SHAPE: sums2 or counts off the 8-byte grid. */
size_t nbp_recon_stats_workspace_bytes(void);
int nbp_recon_stats_f64(const float* d2, long long n, const long long* n_dev_or_null, int T, const float* thresholds_host,
                        double* sums2, long long* counts, void* ws, size_t ws_bytes, void* stream);

/* Per-step reconstruction curve: the same metrics after every step, updated incrementally (the cloud is append-only, the GT fixed).
 * n <= 16 items (HOST arrays of n entries) in THREE launches whatever n: one walk over the items' new points, the partial sums, the
 * items' rows.  Item i: plans[i] = an nbp_nn_plan_build_f32 plan of its G[i] GT points inside lo / hi [n][3] with cell[i] (the plan's
 * fourth float4 component carries the GT index); cloud3[i] = [capacity[i]][3]; count_dev[i] = the cloud's int64 device size;
 * seen_dev[i] = int64 device watermark.  The call reads cloud rows [seen, min(count, capacity)) only -- both ends on the device --
 * and then sets seen = min(count, capacity); seen >= count: nothing new, the row repeats the totals and nothing else moves.
 * d2_gt[i] fp32 [G[i]] in the GT's order: the running truncated squared distance GT -> cloud, initialised by the caller to
 * fl(cap cap), lowered by an integer atomicMin on the bit pattern (exact, and the same bits in every run); d2_new[i] fp32
 * [capacity[i]]: scratch for the new points' own distances; totals[i]: nbp_recon_curve_totals_bytes() bytes, zeroed by the caller
 * at a reset (running accuracy sums and counts); T[i] thresholds in thresholds_host [n][8]; row[i] float64 [6 + 2 T[i]] = (acc
 * sums 2, comp sums 2, n_rec, G, acc counts T, comp counts T); new_bound[i] = host bound of the new points: it only sizes the grid.
 * The completeness half of a row is bit for bit nbp_recon_stats_f64 of d2_gt (the same geometry); batching changes no bit of any
 * item.  ws: nbp_recon_curve_workspace_bytes(n).  No allocation, no host synchronisation.  NBP_E_ARG / NBP_E_SHAPE as above; totals,
 * row, seen or count off the 8-byte grid is NBP_E_SHAPE. */
size_t nbp_recon_curve_workspace_bytes(int n);
size_t nbp_recon_curve_totals_bytes(void);
int nbp_recon_curve_update_batch_f32(int n, const void* const* plans, const int* G, const float* lo_host, const float* hi_host,
                                     const float* cell, const float* cap, const float* const* cloud3, const long long* capacity,
                                     const long long* const* count_dev, long long* const* seen_dev, float* const* d2_gt,
                                     float* const* d2_new, void* const* totals, const int* T, const float* thresholds_host,
                                     double* const* row, const long long* new_bound, void* ws, size_t ws_bytes, void* stream);

/* ---- Cloud-to-mesh accuracy (csrc/nbp_surface.hip).  Not in the reference: the exact truncated squared distance
 * from a point to the GT MESH, fp32, through a uniform grid of triangles.  The definition of record is
 * nextbestpath_amd/utility/surface_metrics.py (point_triangle_d2, mesh_dist2_reference), which the kernels equal bit for bit; the
 * summary of the distances is nbp_recon_stats_f64.  Host binding: hipops.MeshPlan / mesh_dist2 / SurfaceMetrics.
 *   d2[i] = min(cap2, min over the PARTICIPATING triangles of point_triangle_d2(q_i, a, b, c)),  cap2 = fl(cap cap).
 * verts3 [V][3] fp32, faces3 [F][3] int32; a triangle participates iff its indices are inside [0, V) and its three vertices lie
 * inside the box (lo <= v <= hi, fp32; a NaN or an infinity is outside).  The grid is the nearest-neighbour grid above (lo_host /
 * hi_host / cell, cells of 1.001 cell, the same limits); a triangle is registered in every cell between the cells of its bounding
 * box's corners.  The number of (triangle, cell) pairs is known on the device only, so a plan is built in two calls:
 *   nbp_mesh_plan_count_f32   counts and scans into `plan` (nbp_mesh_plan_bytes; ws: nbp_mesh_plan_workspace_bytes), copies the
 *                             participating triangles' vertices there, and leaves totals2_dev [2] int64 = (pairs, participating
 *                             triangles) on the device: the caller reads the first back -- the one host synchronisation of this
 *                             path, at setup -- and allocates `entries` int32 [pairs] (at least one element)
 *   nbp_mesh_plan_fill_i32    writes the pairs' triangle indices into entries; nothing at or beyond entry_capacity is written.
 *                             NBP_E_SHAPE: entry_capacity > 2^31 - 1
 *   nbp_mesh_dist2_planned_f32  one launch: the query walks the shells of cells around its unclamped cell and stops after shell r
 *                             once best <= fl(r cell)^2; the box term of point_triangle_d2 makes that exit exact for triangles of
 *                             any size (the file's header).  Q / Q_dev_or_null as above; a query more than ceil(cap / cell) cells
 *                             outside the grid, or with a NaN, gets cap2 without a memory access.  No atomics on the output.
 * No allocation; no host synchronisation inside the library.  NBP_E_ARG / NBP_E_SHAPE / NBP_E_WS as for nbp_nn_*; totals2_dev off the
 * 8-byte grid is NBP_E_SHAPE.  The size queries return 0 where the call would fail.  F = 0, V = 0 and Q = 0 are legal. */
size_t nbp_mesh_plan_bytes(const float* lo_host, const float* hi_host, float cell, long long F);
size_t nbp_mesh_plan_workspace_bytes(const float* lo_host, const float* hi_host, float cell);
int nbp_mesh_plan_count_f32(const float* verts3, long long V, const int* faces3, long long F, const float* lo_host,
                            const float* hi_host, float cell, void* plan, size_t plan_bytes, long long* totals2_dev, void* ws,
                            size_t ws_bytes, void* stream);
int nbp_mesh_plan_fill_i32(const float* verts3, long long V, const int* faces3, long long F, const float* lo_host,
                           const float* hi_host, float cell, const void* plan, int* entries, long long entry_capacity, void* ws,
                           size_t ws_bytes, void* stream);
int nbp_mesh_dist2_planned_f32(const void* plan, const int* entries, const float* lo_host, const float* hi_host, float cell,
                               float cap, const float* q3, long long Q, const long long* Q_dev_or_null, float* d2, void* stream);

/* ---- The replay store's container in LMDB's on-disk format (csrc/nbp_mdb.cpp; host only).  The reference keeps its experience
 * records in an LMDB environment (next_best_path/trainers/train_nbp_model.py:61-63 lmdb.open(path, map_size);
 * next_best_path/utility/nbp_utils.py:32-141: txn.put per record, ordered cursors, txn.delete of the validation records).  liblmdb is
 * not in this image: these entry points read and write <dir>/data.mdb in LMDB 0.9's file format (4096-byte pages, unnamed main
 * database, memcmp key order, overflow pages for records > 2038 bytes), so that a store written here opens with lmdb and one written
 * by the reference opens here.  One writer; every put / del is its own committed transaction.  Parity unpinned against liblmdb.
 *   nbp_mdb_open     creates <dir> and an empty environment, or loads an existing one (NBP_E_SHAPE: not an LMDB file of this shape --
 *                    other page size, named or duplicate-key databases); sync_each_commit: fdatasync before and after each meta write
 *   nbp_mdb_put      insert or replace; nbp_mdb_del: 0 deleted, 1 not found; nbp_mdb_get: 0 found (*vlen_out = size; the bytes are
 *                    copied when cap >= size), 1 not found
 *   nbp_mdb_keys     every key in order, packed [u16 length][bytes]...; *needed_out = packed size (cap = 0 sizes the buffer)
 *   nbp_mdb_stat     {depth, branch pages, leaf pages, overflow pages, entries, last page, txnid, page size}                          */
int nbp_mdb_open(const char* dir_path, unsigned long long map_size, int sync_each_commit, void** env_out);
int nbp_mdb_close(void* env);
long long nbp_mdb_entries(void* env);
int nbp_mdb_put(void* env, const void* key, size_t klen, const void* val, size_t vlen);
int nbp_mdb_del(void* env, const void* key, size_t klen);
int nbp_mdb_get(void* env, const void* key, size_t klen, void* buf, size_t cap, size_t* vlen_out);
int nbp_mdb_keys(void* env, void* buf, size_t cap, size_t* needed_out);
int nbp_mdb_stat(void* env, unsigned long long* out8);

/* ---- The seeded depth-sensor noise model (csrc/nbp_depth_noise.hip; the definition, which the kernel equals bit for bit, is
 * nextbestpath_amd/utility/depth_noise.py).  Not in the reference.  Clean [H][W] fp32 frames (z = -1: no return) ->
 * noisy frames: axial noise zn = max(z + (sigma_base + sigma_quad z z) g, z_min) with g a 16-byte Irwin-Hall stand-in for a
 * Gaussian, dropout (pixel dropped iff its fifth word < drop_thr; 0 = off) and, for edge_threshold > 0, flying-pixel dropout
 * against the clean 4-neighbours; dropped and background pixels come out at -1.  A frame's noise depends on (seed, frame id, pixel)
 * only.  Out of place: a clean frame that overlaps an output frame is NBP_E_ARG.  One launch, no workspace, no atomics.
 *   nbp_depth_noise_f32        n (<= 65535) consecutive frames of one camera; frame i has id first_frame + i (mod 2^32)
 *   nbp_depth_noise_batch_f32  n (<= 48: 12 items of <= 4 frames) frames, each with its own clean / out pointer, seed and frame id
 *                              (HOST arrays of n entries; they travel as kernel arguments)
 * 16-byte accesses when W % 4 == 0 and every frame lies on the 16-byte grid, 4-byte accesses otherwise: any H, W >= 1.
 * NBP_E_ARG: null pointer, n / H / W < 1, a negative or NaN parameter, z_min <= 0, overlapping frames; NBP_E_SHAPE: H W > 2^29 or
 * more frames than the form takes.  Nothing is written on an error. */
int nbp_depth_noise_f32(const float* clean, float* out, int n, int H, int W, unsigned seed, unsigned first_frame, float sigma_base,
                        float sigma_quad, float z_min, unsigned drop_thr, float edge_threshold, void* stream);
int nbp_depth_noise_batch_f32(int n, const float* const* clean, float* const* out, const unsigned* seeds, const unsigned* frames,
                              int H, int W, float sigma_base, float sigma_quad, float z_min, unsigned drop_thr, float edge_threshold,
                              void* stream);

/* ---- The depth-frame filter (csrc/nbp_depth_filter.hip; the definition, which the kernel equals bit for bit, is
 * nextbestpath_amd/utility/depth_filter.py).  Not in the reference.  Raw [H][W] fp32 frames (z = -1: no return; a
 * pixel is valid iff z > -1) -> filtered frames, in one pass that reads the raw frame only; every output value is an element of
 * the input or -1.  Window: the (2 radius + 1)^2 - 1 neighbours inside the image; gate(c) = range_base + range_quad (c c), three
 * fp32 operations.  Valid centre z: n = the valid neighbours with |z_q - z| <= gate(z); n < min_support -> -1; else, smooth != 0 ->
 * the element of rank n / 2 of those neighbours and z (the median, the lower one of an even set); else z.  Invalid centre,
 * fill_support > 0 and at least fill_support valid neighbours: m = their element of rank (count - 1) / 2, written iff every one of
 * them has |v - m| <= gate(m); -1 otherwise.  Out of place: a raw frame that overlaps an output frame is NBP_E_ARG.  One launch
 * (a 32 x 32 tile with its halo in LDS per workgroup), no workspace, no atomics.
 *   nbp_depth_filter_f32        n (<= 65535) consecutive frames
 *   nbp_depth_filter_batch_f32  n (<= 48: 12 items of <= 4 frames) frames, each with its own raw / out pointer (HOST arrays of n
 *                               entries; they travel as kernel arguments)
 * 16-byte accesses when W % 4 == 0 and every frame lies on the 16-byte grid, 4-byte accesses otherwise: any H, W >= 1.
 * NBP_E_ARG: null pointer, n / H / W < 1, radius not 1 or 2, a negative or NaN range, both ranges 0, a support outside
 * 0 .. (2 radius + 1)^2 - 1, overlapping frames; NBP_E_SHAPE: H W > 2^29 or more frames than the form takes.  Nothing is written
 * on an error. */
int nbp_depth_filter_f32(const float* raw, float* out, int n, int H, int W, int radius, float range_base, float range_quad,
                         int smooth, int min_support, int fill_support, void* stream);
int nbp_depth_filter_batch_f32(int n, const float* const* raw, float* const* out, int H, int W, int radius, float range_base,
                               float range_quad, int smooth, int min_support, int fill_support, void* stream);

/* ---- Held-out view metrics (csrc/nbp_views.hip; the definition, which the kernels equal, is
 * nextbestpath_amd/utility/view_metrics.py).  Not in the reference.  A point-splat render of a cloud [n][3] that is on
 * the device from n_views cameras (cams_host [n_views][12]: R row-major then T, on the HOST; they travel as kernel arguments in
 * chunks of 8), and its comparison with a mesh render of the same cameras.
 *   nbp_views_splat_f32   keys [n_views][H][W] uint64: per pixel the smallest (float bits of v2) << 32 | point index over the points
 *                         whose (2 radius + 1)^2 footprint, clipped to the image, holds the pixel; ~0 = empty.  A point takes part iff
 *                         z_clip < v2 < z_far and its NDC coordinates are finite; its pixel is the inverse of the un-projection's NDC
 *                         tables in fp32 (view_metrics.project, bit for bit).  n: host bound of the rows, and the int64 device counter
 *                         where given (rows at or beyond it are never read).  The call sets the keys to ~0 first unless accumulate
 *                         != 0; the merge is a 64-bit atomicMin, behind a plain load that skips it where the stored key is already
 *                         lower (precheck != 0; 0 = every pixel goes to the atomic: the same bits).  A minimum is order-free: two
 *                         runs give the same bits, and so does a cloud splatted in parts into the same keys -- each part at its
 *                         own row positions in cloud3 (the index in a key is the row; there is no first-index argument: rows
 *                         that are not part of a call are masked with NaN, or lie beyond its count).  One launch per 8 views.
 *   nbp_views_resolve_f32 the rendered images: z_c [n_views][H][W] (-1 where empty), rgb_c [..][3] = cloud_rgb[index] (0 where
 *                         empty), index int64 (-1 where empty); each output may be null.  n_cloud = rows of the cloud the keys were
 *                         made from (and of cloud_rgb): a key whose index is at or beyond it reads as empty, never as an address.
 *   nbp_views_stats_f64   resolve + classify + reduce in two launches of a fixed geometry (per-thread strided partials, a fixed tree
 *                         in the block, one stored row per block, rows added in index order; no floating-point atomics: two runs give
 *                         the same bits).  With gt = z_gt > -1 and z_gt < z_far, c = pixel not empty, dz = z_c - z_gt in fp32:
 *                         counts6 [n_views][6] int64 = n_gt, n_c, n_hit (gt, c, |dz| <= tol), n_hole (gt, not c), n_leak (gt, c,
 *                         dz > tol), n_floater (c and (not gt or dz < -tol)); sums3 [n_views][3] float64 over the hit pixels = sum
 *                         |dz|, sum dz^2, squared colour error over the three channels (differences in float64 from the fp32 values;
 *                         0 where cloud_rgb or rgb_gt is null).  ws: nbp_views_stats_workspace_bytes(n_views) (0 where it would fail).
 * No allocation, no host synchronisation.  NBP_E_ARG: a null pointer, n_views < 1, H or W < 2, radius outside 0..4, a negative count,
 * a tolerance that is negative or not finite, in the splat tan_half_fov <= 0, z_clip <= 0 or z_far <= z_clip, in the statistics
 * (which take no z_clip) z_far <= 0; NBP_E_SHAPE: H W > 2^29, a cloud of 2^32 - 1 points or more (the key's
 * low word is the index), more than 65535 views in the statistics, keys / index / counts6 / sums3 off the 8-byte grid; NBP_E_WS.
 * Nothing is written on an error. */
int nbp_views_splat_f32(const float* cloud3, long long n, const long long* n_dev_or_null, const float* cams_host, int n_views, int H,
                        int W, int radius, float tan_half_fov, float z_clip, float z_far, int accumulate, int precheck,
                        unsigned long long* keys, void* stream);
int nbp_views_resolve_f32(const unsigned long long* keys, const float* cloud_rgb_or_null, long long n_cloud, int n_views, int H, int W,
                          float* z_c_or_null, float* rgb_c_or_null, long long* index_or_null, void* stream);
size_t nbp_views_stats_workspace_bytes(int n_views);
int nbp_views_stats_f64(const unsigned long long* keys, const float* cloud_rgb_or_null, long long n_cloud, const float* z_gt,
                        const float* rgb_gt_or_null, int n_views, int H, int W, float depth_tolerance, float z_far,
                        long long* counts6, double* sums3, void* ws, size_t ws_bytes, void* stream);

/* ---- Frontier-based exploration as a policy behind the network's interface (csrc/nbp_frontier.hip; the definition, which the
 * kernels equal bit for bit, is nextbestpath_amd/utility/frontier.py).  Not in the reference.  maps6 [B][6][S][S] fp32,
 * S a multiple of 64, V = S / 4, W = S / 64.  Bit i of word w of a packed row is column 64 w + i.
 *   nbp_frontier_workspace_bytes  what the policy call needs (5 B S W words; the mask call needs four of the five); 0 where the
 *                                 call would fail.
 *   nbp_frontier_mask_u64         frontier_bits [B][S][W]: the free pixels with an unknown edge neighbour (unknown = outside the
 *                                 closing of `seen` by a (2 dilate + 1)-square); unknown_bits (same shape, may be null): the unknown
 *                                 pixels.  Four launches.
 *   nbp_frontier_policy_f32       out1 [B][8][V][V] = float(max(gain - distance_penalty max(|g0 - V/2|, |g1 - V/2|), 0)), gain = the
 *                                 frontier pixels within `radius` of pixel (4 g0, 4 g1) in the 45-degree sector of the heading;
 *                                 out2 [B][1][S][S] = 1 at the unknown pixels where unknown_obstacle != 0, else 0.  Both are written
 *                                 completely.  Five launches (one more per 2^24 gain workgroups).
 * No atomics, no hand-off between workgroups: two runs give the same bits.  No allocation, no host synchronisation; any B >= 1.
 * NBP_E_ARG: a null pointer (but unknown_bits), B < 1, S < 1, radius outside 1..31, dilate outside 0..8, distance_penalty < 0;
 * NBP_E_SHAPE: S % 64 != 0, frontier_bits / unknown_bits / ws off the 8-byte grid; NBP_E_WS.  Nothing is launched on an error. */
size_t nbp_frontier_workspace_bytes(int B, int S);
int nbp_frontier_mask_u64(const float* maps6, int B, int S, int dilate, unsigned long long* frontier_bits,
                          unsigned long long* unknown_bits_or_null, void* ws, size_t ws_bytes, void* stream);
int nbp_frontier_policy_f32(const float* maps6, int B, int S, int radius, int dilate, int unknown_obstacle, int distance_penalty,
                            float* out1, float* out2, void* ws, size_t ws_bytes, void* stream);

/* ---- Next-best-view by ray-cast information gain as a policy behind the network's interface (csrc/nbp_infogain.hip; the definition,
 * which the kernels equal bit for bit, is nextbestpath_amd/utility/infogain.py).  Not in the reference.  maps6, S, V, W
 * and the packed rows as for nbp_frontier_*; pack, dilate and erode are that path's launches.
 *   nbp_infogain_workspace_bytes  what either call needs (4 B S W words); 0 where the call would fail.
 *   nbp_infogain_policy_f32       out1 [B][8][V][V] = float(max(gain - distance_penalty max(|g0 - V/2|, |g1 - V/2|), 0)), gain = the
 *                                 unknown pixels within `radius` of pixel (4 g0, 4 g1), in the 45-degree sector of the heading, that
 *                                 a ray of the 8 `radius`-ray fan reaches from that pixel before a blocked pixel (occupied, or outside
 *                                 the domain of rows and columns >= 1) or a diagonal step between two blocked corners stops it;
 *                                 out2 [B][1][S][S] = 1 at the unknown pixels where unknown_obstacle != 0, else 0.  Both are written
 *                                 completely.  Five launches; one wave per value cell.
 *   nbp_infogain_visible_u64      the visible masks of chosen cells, to locate a gain mismatch: cells_host [n][3] = (b, g0, g1) in
 *                                 HOST memory (read before the call returns); out [n][2 radius + 1] words, bit dx + radius of word
 *                                 dy + radius = pixel (4 g0 + dy, 4 g1 + dx) is visible.  Three launches and one per 128 cells.
 * Integer ORs in LDS only; no global atomics, no floating-point atomics, no hand-off between workgroups: two runs give the same bits.
 * No allocation, no host synchronisation; any B >= 1.
 * NBP_E_ARG: a null pointer, B < 1, S < 1, radius outside 1..31, dilate outside 0..8, distance_penalty < 0, n < 1, a cell with b outside
 * 0..B-1 or g0, g1 outside 0..V-1; NBP_E_SHAPE: S % 64 != 0, out (of the visible call) / ws off the 8-byte grid; NBP_E_WS.  Nothing is
 * launched on an error. */
size_t nbp_infogain_workspace_bytes(int B, int S);
int nbp_infogain_policy_f32(const float* maps6, int B, int S, int radius, int dilate, int unknown_obstacle, int distance_penalty,
                            float* out1, float* out2, void* ws, size_t ws_bytes, void* stream);
int nbp_infogain_visible_u64(const float* maps6, int B, int S, int radius, int dilate, const int* cells_host, int n,
                             unsigned long long* out, void* ws, size_t ws_bytes, void* stream);

/* ---- TSDF fusion of depth frames, and the fused surface cloud (csrc/nbp_tsdf.hip; the definition, which the kernels equal bit for
 * bit, is nextbestpath_amd/utility/tsdf.py).  Not in the reference.  A volume is int32 [nx][ny][nz][2] on the device:
 * voxel (i, j, k), linear index (i ny + j) nz + k, holds (S, W) = (sum of quantised signed distances, number of observations); its
 * centre on axis a is lo_a + (f32(i_a) + 0.5) voxel.  lo_host [3], the cameras ([.][12]: R row-major then T) and the pointer tables
 * are HOST memory, read before the call returns; they travel as kernel arguments.
 *   nbp_tsdf_integrate_f32        n (<= 65535) [H][W] fp32 frames into ONE volume: consecutive in depth_or_null, or each at its own
 *                                 address frames_host_or_null[n] (exactly one of the two is given); cams_host [n][12].  A frame
 *                                 updates a voxel iff the centre projects (view_metrics.project with this z_clip and tan_half_fov)
 *                                 onto a pixel of the image whose depth d has d > -1 (a NaN has not) and d <= max_depth, and sdf = d -
 *                                 v2 >= -trunc: S += (int) rint(min(sdf, trunc) (127 / trunc)), W += 1.  One launch per 4 frames.
 *   nbp_tsdf_integrate_batch_f32  n_items (<= 12) volumes, item i with its own vols_host[i], lo_host [i][3], voxel_host[i],
 *                                 dims_host [i][3] = nx, ny, nz, trunc_host[i], max_depth_host[i] and n_frames_host[i] (1..4) frames
 *                                 frames_host [i][4] with cams_host [i][4][12], all frames [H][W].  ONE launch; each volume gets the
 *                                 bits of a call of its own.
 *                                 A thread owns a voxel, loads (S, W) once, loops over the launch's frames in registers and stores
 *                                 once, and only where a frame updated it.  No atomics: integer sums with one owner, so frames in any
 *                                 order or grouping give the same bits.
 *   nbp_tsdf_extract_f32          the fused surface cloud, points [.][3] in the order (linear index, axis 0, 1, 2): voxel and its
 *                                 neighbour one step up the axis both usable (W >= min_weight and |S| < 127 W) and (S0 < 0) != (S1 <
 *                                 0) -> the voxel's centre with (D0 / (D0 - D1)) voxel added on that axis, D = f32(S) / f32(W).
 *                                 total (int64, device) receives the number of points whatever the capacity; the first `capacity`
 *                                 rows are written, nothing beyond them (capacity 0: points may be null, the count alone).  Three
 *                                 launches (count per run of voxels, scan, emit); ws: nbp_tsdf_extract_workspace_bytes(nx ny nz)
 *                                 (0 where the call would fail).
 *   nbp_tsdf_stats_i64            counts2 (int64 [2], device) = #(W > 0), #usable.  Two launches of a fixed geometry; ws:
 *                                 nbp_tsdf_stats_workspace_bytes().
 * No allocation, no host synchronisation; two runs give the same bytes.  NBP_E_ARG: a null pointer, n / n_items / a frame count / a
 * dimension / H / W < 1, voxel, trunc, tan_half_fov or z_clip not positive and finite, lo not finite, max_depth not positive (it may
 * be infinite), min_weight < 1, capacity < 0, both or neither of depth and frames_host, a frame (or the extraction's points, total or
 * workspace) that overlaps a volume, two overlapping volumes in one batch; NBP_E_SHAPE: more than 2^28 voxels, H W > 2^29, more frames
 * or items than the form takes, a volume, total or counts2 off the 8-byte grid; NBP_E_WS.  Nothing is written on an error. */
int nbp_tsdf_integrate_f32(int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, const float* depth_or_null,
                           const float* const* frames_host_or_null, int n, const float* cams_host, int H, int W, float tan_half_fov,
                           float z_clip, float trunc, float max_depth, void* stream);
int nbp_tsdf_integrate_batch_f32(int n_items, int* const* vols_host, const float* lo_host, const float* voxel_host, const int* dims_host,
                                 const float* trunc_host, const float* max_depth_host, const int* n_frames_host,
                                 const float* const* frames_host, const float* cams_host, int H, int W, float tan_half_fov,
                                 float z_clip, void* stream);
size_t nbp_tsdf_extract_workspace_bytes(long long n_voxels);
int nbp_tsdf_extract_f32(const int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, int min_weight,
                         float* points_or_null, long long capacity, long long* total, void* ws, size_t ws_bytes, void* stream);
size_t nbp_tsdf_stats_workspace_bytes(void);
int nbp_tsdf_stats_i64(const int* vol, long long n_voxels, int min_weight, long long* counts2, void* ws, size_t ws_bytes, void* stream);

/* ---- a triangle mesh out of the TSDF volume, by naive surface nets (csrc/nbp_tsdf_mesh.hip; the definition, which the kernels equal
 * bit for bit, is nextbestpath_amd/utility/tsdf_mesh.py).  Not in the reference.  The volume, lo_host and min_weight
 * are nbp_tsdf_extract_f32's.
 *   nbp_tsdf_mesh_f32             one vertex per grid cell (its low corner voxel's linear index is the cell's) that holds a crossing
 *                                 of the extraction: the mean of the cell's crossing points, added in edge order from +0; verts
 *                                 [.][3] in cell order.  One quad per crossing (v, a) with 1 <= v[b], v[c] <= dims - 2 on the other
 *                                 two axes: the vertex ids (ranks in verts) of the four cells around the edge, turning from axis (a +
 *                                 1) % 3 to (a + 2) % 3 where S0 < 0 and the other way round otherwise, as the triangles (r0, r1,
 *                                 r2), (r0, r2, r3); faces [.][3] int32 in the extraction's order, area2 [.] (may be null) = 0.25
 *                                 |cross(v1 - v0, v2 - v0)|^2 per face.  totals2 (int64 [2], device) receives the numbers of
 *                                 vertices and of faces whatever the capacities; the first vert_capacity / face_capacity rows are
 *                                 written, nothing beyond them (a face is written whatever ids it holds); both capacities 0: the
 *                                 counts alone, the buffers may be null.  Two launches to count (per run of voxels, scan), one for
 *                                 the vertices, one for the faces; ws: nbp_tsdf_mesh_workspace_bytes(nx ny nz) (0 where the call
 *                                 would fail): the runs' offsets and an int32 vertex id per voxel.
 * No allocation, no host synchronisation, no atomics; two runs give the same bytes.  NBP_E_ARG: a null volume, lo, totals2 or
 * workspace, a null buffer with a capacity above 0, a dimension or min_weight < 1, a capacity < 0, voxel not positive and finite, lo
 * not finite, two of the volume, totals2, the workspace and the outputs overlapping; NBP_E_SHAPE: more than 2^28 voxels, the volume
 * or totals2 off the 8-byte grid; NBP_E_WS.  Nothing is written on an error. */
size_t nbp_tsdf_mesh_workspace_bytes(long long n_voxels);
int nbp_tsdf_mesh_f32(const int* vol, const float* lo_host, float voxel, int nx, int ny, int nz, int min_weight, float* verts_or_null,
                      long long vert_capacity, int* faces_or_null, float* area2_or_null, long long face_capacity, long long* totals2,
                      void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NBP_HIP_H */
