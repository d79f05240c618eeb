/*
 * gdl_hip.h -- C ABI of libgdl_hip.so: the MI355X (gfx950) implementation of the
 * DGL audio-visual training step of shicaiwei123/ICCV2025-GDL (main_dgl.py:90-162).
 *
 * Conventions (every entry point):
 *   - plain C, raw DEVICE pointers, explicit sizes; no torch / C++ types;
 *   - returns 0 on success, a GDL_ERR_* code otherwise; gdl_last_error() gives a
 *     thread-local message; nothing throws across the boundary;
 *   - never allocates or frees device memory: workspaces are caller-provided and
 *     sized by the *_workspace_bytes query;
 *   - never synchronises the device: work is enqueued on the hipStream_t passed
 *     (as void*); the library keeps no pointer after return except inside an
 *     explicitly created gdl_encoder_t / gdl_optim_t object.
 *
 * Activations inside the library are NHWC in `dtype` (GDL_BF16 for the benchmark
 * configuration, GDL_F32 for the exact-f32 parity mode).  Parameters, gradients,
 * BatchNorm statistics, pooled features, logits and losses are float32 in the
 * reference's own layouts (conv weight [K][C][R][S], linear weight [out][in]).
 *
 * Reference interface each group replaces is cited as file:line into
 * /root/reference (the PyTorch operators the reference calls there).
 */
#ifndef GDL_HIP_H
#define GDL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDL_API __attribute__((visibility("default")))

enum { GDL_OK = 0, GDL_ERR_ARG = 1, GDL_ERR_HIP = 2, GDL_ERR_STATE = 3, GDL_ERR_WORKSPACE = 4 };
enum { GDL_F32 = 0, GDL_BF16 = 1 };
enum { GDL_AUDIO = 0, GDL_VISUAL = 1 };

GDL_API const char* gdl_last_error(void);
GDL_API int gdl_version(void);
/* number of compute units / device name of the current device (host query) */
GDL_API int gdl_device_info(int* cu_count, char* name, int name_len);

/* ------------------------------------------------------------------ convolution
 * nn.Conv2d(bias=False): backbone.py:20-23 (3x3 s1/s2 p1), :26-28 (1x1 s2),
 * :96-101 (7x7 s2 p3 stem).  Implicit GEMM on MFMA.
 *
 * gdl_conv_fwd:  x NHWC [N][H][W][C] (dtype), w_krsc [K][R][S][C] (dtype, from
 *   gdl_pack_weight) -> y NHWC [N][P][Q][K] (dtype).  C % (128/sizeof(dtype)) == 0,
 *   K % 64 == 0.  If bn_partial != NULL the epilogue also writes per-channel
 *   (sum, sum of squares) of the STORED values of each M-tile:
 *   bn_partial[tile][K][2] float, tile < gdl_conv_bn_tiles(...).
 * gdl_conv_dgrad: dy [N][P][Q][K], w_crsk [C][R][S][K] -> dx [N][H][W][C]
 *   (+ addend, same shape as dx, may alias dx; NULL for none).
 * gdl_conv_wgrad: dy, x -> dw [K][C][R][S] float32 (overwritten).  `ws` holds
 *   split-K partials; size from gdl_conv_wgrad_workspace_bytes.
 */
/* Gather tables: every conv kernel addresses its gathered operand as table[m].off0 + delta[tap]
 * (8 bytes per GEMM row: byte offset of tap 0 + a validity bit per tap), so the K-loops carry no
 * division / multiplication / bounds arithmetic.  Built once per geometry:
 *   mode GDL_GATHER_FWD   rows = output pixels; used by gdl_conv_fwd and gdl_conv_wgrad
 *   mode GDL_GATHER_DGRAD rows = input pixels;  used by gdl_conv_dgrad */
enum { GDL_GATHER_FWD = 0, GDL_GATHER_DGRAD = 1 };
GDL_API size_t gdl_conv_table_bytes(int mode, int N, int H, int W, int R, int S, int stride, int pad);
GDL_API int gdl_conv_build_table(int mode, int dtype, int N, int H, int W, int C, int K, int R, int S, int stride,
                                 int pad, void* table, void* stream);
GDL_API int gdl_conv_bn_tiles(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
GDL_API int gdl_conv_fwd(int dtype, const void* x, const void* w_krsc, void* y, float* bn_partial, const void* table,
                         int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream);
GDL_API int gdl_conv_dgrad(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend,
                           const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                           void* stream);
/* ReLU backward folded into the data gradient (BasicBlock: out = relu(bn2(conv2(..)) + identity), backbone.py:62-66).
 * gdl_bn_act_bits = gdl_bn_act(relu = 1) that also stores the sign bits of its output, one byte per 16-byte vector
 * (bit e = element e > 0); gdl_conv_dgrad_relu = gdl_conv_dgrad whose stored result (dx + addend) is zeroed where the
 * bit of the tensor it is the gradient of is 0 -- the next block's backward then needs neither that tensor nor a
 * separate masking pass. */
GDL_API int gdl_bn_act_bits(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                            const float* res_scale, const float* res_shift, void* out, uint8_t* relu_bits, size_t M, int C,
                            void* stream);
GDL_API int gdl_conv_dgrad_relu(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend,
                                const uint8_t* relu_bits, const void* table, int N, int H, int W, int C, int K, int R, int S,
                                int stride, int pad, void* stream);
/* gdl_conv_fwd with the epilogue's optional extras: y = conv(x, w) + bias[K] (float32) + addend (like y), and
 * gelu_out = gelu(y) (exact erf form, of the value as stored) -- nn.Linear with its bias, the residual connection of a Swin
 * block, Mlp.fc1 + act in one launch (swin_transformer.py:26-42, 150-152, 287-290), R = S = 1. */
GDL_API int gdl_conv_fwd_bias(int dtype, const void* x, const void* w_krsc, void* y, const float* bias, const void* addend,
                              void* gelu_out, const void* table, int N, int H, int W, int C, int K, int R, int S, int stride,
                              int pad, void* stream);
/* First block of layers 2-4 (backbone.py:119-124, 141-146: conv1 is 3x3 stride 2, the shortcut a 1x1 stride-2 conv +
 * BatchNorm): the gradient of the block input is the sum of two data gradients,
 *   dx = conv1^T(dy [N][P][Q][K], w_crsk [C][3][3][K]) + downsample^T(dy_ds [N][P][Q][K], w_ds_ck [C][K]),
 * computed in ONE launch (the shortcut is one more tap of the (even, even) input pixels); relu_bits optional as in
 * gdl_conv_dgrad_relu.  `table` = the GDL_GATHER_DGRAD table of the 3x3 stride-2 pad-1 geometry. */
GDL_API int gdl_conv_dgrad_ds(int dtype, const void* dy, const void* w_crsk, const void* dy_ds, const void* w_ds_ck, void* dx,
                              const uint8_t* relu_bits, const void* table, int N, int H, int W, int C, int K, void* stream);
/* BatchNorm-backward reductions in the producing data gradient's epilogue (round 3).  BasicBlock backward (backbone.py:52-66
 * through autograd): the gradient dx a data gradient writes flows into a BatchNorm backward, which first needs per channel
 *   sum g'  and  sum g' * (y - mean) * rstd,   g' = dx as stored (after the addend and the relu_bits mask),
 * y = that BatchNorm's saved input.  gdl_conv_dgrad_bn = gdl_conv_dgrad(_relu) whose epilogue also leaves those sums per M-tile,
 * partial[tile][C][2] (tile < gdl_conv_dgrad_bn_tiles(...)), ready for gdl_bn_bwd_finalize -- the separate reduce pass over
 * g and y (gdl_bn_bwd_reduce: two tensor reads) disappears.  y2 / mean2 / rstd2 / partial2 (all or none): a second BatchNorm
 * fed by the same gradient (the downsample branch's; not with the 64 -> 64 channel persistent kernel). */
GDL_API int gdl_conv_dgrad_bn_tiles(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
GDL_API int gdl_conv_dgrad_bn(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend,
                              const uint8_t* relu_bits, const void* table, int N, int H, int W, int C, int K, int R, int S,
                              int stride, int pad, const void* y, const float* mean, const float* rstd, float* partial,
                              const void* y2, const float* mean2, const float* rstd2, float* partial2, void* stream);
/* Split-K of the 3x3 stride-1 "slab" convolutions (round 3).  Where a layer's output tiles would leave most CUs idle (layer 4
 * of both encoders: 3 456 / 9 408 GEMM rows against a 4 608-deep reduction; the audio layer 3), 2 or 4 blocks share a tile, each
 * multiplies a slice of the input channels and leaves fp32 accumulators in `split_ws`; a finish kernel folds them in fixed order
 * (run-to-run identical) and applies the epilogue -- rounding, addend, ReLU bits, BatchNorm statistics / BatchNorm-backward sums,
 * the same partial-row counts as the unsplit forms.  gdl_conv_split_workspace_bytes: bytes a geometry needs (0: it does not
 * split; dgrad = 0 forward, 1 data gradient).  The _split entry points equal gdl_conv_fwd / gdl_conv_dgrad_bn with that workspace
 * (NULL or too small: refused / unsplit).  bf16 only; results differ from the unsplit kernel by fp32 summation order. */
GDL_API size_t gdl_conv_split_workspace_bytes(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                              int dgrad);
GDL_API int gdl_conv_fwd_split(int dtype, const void* x, const void* w_krsc, void* y, float* bn_partial, const void* table, int N,
                               int H, int W, int C, int K, int R, int S, int stride, int pad, void* split_ws,
                               size_t split_ws_bytes, void* stream);
GDL_API int gdl_conv_dgrad_bn_split(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend,
                                    const uint8_t* relu_bits, const void* table, int N, int H, int W, int C, int K, int R, int S,
                                    int stride, int pad, const void* y, const float* mean, const float* rstd, float* partial,
                                    const void* y2, const float* mean2, const float* rstd2, float* partial2, void* split_ws,
                                    size_t split_ws_bytes, void* stream);
/* Mlp backward in the data gradient's epilogue (round 3; /root/reference/models/swin_transformer.py:32-47, Mlp.forward
 * fc1 -> act -> fc2 through autograd): gdl_conv_dgrad_gelu = gdl_conv_dgrad whose epilogue multiplies the stored value by
 * gelu'(u[row][c]) (u laid out like dx: fc1's biased output, as gdl_conv_fwd_bias left it) and adds the column sums of dx AS
 * STORED -- fc1's bias gradient -- to `acc`, int64 [C][2] fixed-point accumulators the caller zeroes: acc[2c] += round(sum *
 * scale) per M-tile with device-scope integer atomics (associative: bit-identical from run to run).  acc[2c + 1] is the channel's overflow / NaN MARK and must be zeroed with the rest: a tile sum that does not fit the channel's share of 2^62 (or is NaN / inf) sets it instead of being added.  Choose scale = 2^(62 - h - ceil(log2(rows))) for |mean| < 2^h.
 * gdl_acc_to_float: out[c] = acc[2c] * inv_scale, or NaN when acc[2c + 1] != 0 (a marked channel) -- not a reader of [sum, sumsq] pairs.  Replaces gdl_swin_colsum(g, u): three passes over the widest tensor of a
 * block. */
GDL_API int gdl_conv_dgrad_gelu(int dtype, const void* dy, const void* w_crsk, void* dx, const void* u, void* acc, double scale,
                                const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                void* stream);
GDL_API int gdl_acc_to_float(const void* acc, int n, double inv_scale, float* out, void* stream);
GDL_API size_t gdl_conv_wgrad_workspace_bytes(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride,
                                              int pad);
GDL_API int gdl_conv_wgrad(int dtype, const void* dy, const void* x, float* dw_kcrs, const void* table, int N, int H,
                           int W, int C, int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes,
                           void* stream);
/* float32 [K][C][R][S] -> dtype [K][R][S][C] (w_krsc) and dtype [C][R][S][K] (w_crsk); either may be NULL */
GDL_API int gdl_pack_weight(int dtype, const float* w_kcrs, void* w_krsc, void* w_crsk, int K, int C, int R, int S,
                            void* stream);


/* Direct (implicit-GEMM) stem, backbone.py:96-101,166 (7x7 stride 2 pad 3) -- what the encoder engine runs.  The reference's
 * input tensor (float32 [B][Cin][T][H][W] visual / [B][1][H][W] audio, read in place through its strides) is copied once
 * into a zero-padded channels-last image with 4 channels per pixel,
 *     xp [B*T][H+6][W+8][4] dtype   (gdl_stem_pad_bytes bytes),
 * in which a filter row of an output pixel is 8 consecutive pixels (64 bytes bf16 / 128 bytes f32).
 * gdl_pack_stem_rows: float32 [64][Cin][7][7] -> dtype [64][taps][IC] (gdl_stem_weight_bytes bytes;
 * one 128-byte K-step = one filter row in f32, two in bf16; padding slots are zero).
 * gdl_stem_build_table: the gather table of the stem (gdl_stem_table_bytes bytes), built once per shape.
 * gdl_stem_conv_fwd: y NHWC [B*T][P][Q][64] dtype (+ BatchNorm partials as gdl_conv_fwd,
 *   tiles = gdl_stem_conv_bn_tiles).  gdl_stem_conv_wgrad: dw [64][Cin][7][7] float32 from dy [M][64]. */
GDL_API size_t gdl_stem_pad_bytes(int dtype, int n_img, int H, int W);
GDL_API size_t gdl_stem_weight_bytes(int dtype);
GDL_API size_t gdl_stem_table_bytes(int n_img, int H, int W);
GDL_API int gdl_stem_pad(int dtype, const float* x, void* xp, int B, int Cin, int T, int H, int W, void* stream);
GDL_API int gdl_pack_stem_rows(int dtype, const float* w, void* wp, int Cin, void* stream);
GDL_API int gdl_stem_build_table(int dtype, int n_img, int H, int W, void* table, void* stream);
GDL_API int gdl_stem_conv_bn_tiles(int dtype, int n_img, int H, int W);
GDL_API int gdl_stem_conv_fwd(int dtype, const void* xp, const void* wp, void* y, float* bn_partial, const void* table,
                              int n_img, int H, int W, int Cin, void* stream);
GDL_API size_t gdl_stem_conv_wgrad_workspace_bytes(int n_img, int H, int W);
GDL_API int gdl_stem_conv_wgrad(int dtype, const void* dy, const void* xp, float* dw, const void* table, int n_img, int H,
                                int W, int Cin, void* ws, size_t ws_bytes, void* stream);
/* Fused stem backward (round 5): gdl_maxpool_bn_bwd_apply (below) and gdl_stem_conv_wgrad in ONE launch -- the max-pool gather, the
 * ReLU mask and the BatchNorm-backward apply of /root/reference/models/backbone.py:104-106 reversed, feeding the weight gradient
 * of the 7x7/2 stem convolution (backbone.py:97-101) tile by tile through LDS: the gradient of the stem output (the largest
 * activation) is never stored.  dout / idx: gradient and arg-max codes of the POOLED map [n_img*P'*Q'][64] (P' x Q' the pooled
 * size of the (H-1)/2+1 x (W-1)/2+1 stem output), y: the stem output, scale .. coef as for gdl_maxpool_bn_bwd_apply, xp: the
 * padded input of gdl_stem_pad, dw [64][Cin][7][7] float32; workspace as gdl_stem_conv_wgrad_workspace_bytes.  bf16 with stem
 * output rows of at least 64 pixels only (gdl_stem_bwd_fused_ok; other shapes run the two launches).  The result is
 * bit-identical to the two-launch form (same element arithmetic, same stages, same fold). */
GDL_API int gdl_stem_bwd_fused_ok(int dtype, int W);
GDL_API int gdl_stem_bwd_fused(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* scale,
                               const float* shift, const float* save_mean, const float* save_rstd, const float* gamma,
                               const float* coef, const void* xp, float* dw, int n_img, int H, int W, int Cin, void* ws,
                               size_t ws_bytes, void* stream);

/* layout conversion at the module boundary: NHWC dtype <-> NCHW float32 */
GDL_API int gdl_nhwc_to_nchw_f32(int dtype, const void* x, float* y, int N, int H, int W, int C, void* stream);
GDL_API int gdl_nchw_f32_to_nhwc(int dtype, const float* x, void* y, int N, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------ BatchNorm2d (+ReLU, +residual)
 * nn.BatchNorm2d(eps 1e-5, momentum 0.1): backbone.py:45,48,104,144; nn.ReLU and
 * `out += identity`: backbone.py:46,57,65-66,105.
 *
 * gdl_bn_finalize_train: reduces conv-epilogue partials [tiles][C][2] over `count`
 *   elements per channel -> save_mean, save_rstd (biased variance), scale =
 *   gamma*rstd, shift = beta - mean*scale; updates running_mean / running_var
 *   (unbiased) with `momentum` and increments *num_batches_tracked (int64) when
 *   the pointers are non-NULL.
 * gdl_bn_finalize_eval: scale/shift from the running statistics.
 * gdl_bn_act: out = [relu]( y*scale+shift + residual ), residual = none |
 *   res (raw tensor) | res*res_scale+res_shift (downsample branch).
 * gdl_bn_stats: per-channel partials of an existing tensor (when the producer
 *   was not gdl_conv_fwd); same partial format, tiles = gdl_bn_stats_tiles(M).
 */
GDL_API int gdl_bn_stats_tiles(int M);
GDL_API int gdl_bn_stats(int dtype, const void* y, float* partial, int M, int C, void* stream);
GDL_API int gdl_bn_finalize_train(const float* partial, int tiles, int C, double count, const float* gamma,
                                  const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, float* save_mean, float* save_rstd, float* scale,
                                  float* shift, void* stream);
GDL_API int gdl_bn_finalize_eval(int C, const float* gamma, const float* beta, float eps, const float* running_mean,
                                 const float* running_var, float* scale, float* shift, void* stream);
GDL_API int gdl_bn_act(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                       const float* res_scale, const float* res_shift, int relu, void* out, size_t M, int C,
                       void* stream);
/* backward.  g = upstream gradient w.r.t. the BN output (after an optional fused
 * ReLU mask: relu_mask != 0 applies (y*scale+shift > 0) to g).
 * gdl_bn_bwd_reduce -> partial[blocks][C][2]; gdl_bn_bwd_finalize -> dgamma, dbeta
 * (float32, overwritten) and coef[2][C] = {dbeta/M, dgamma/M};
 * gdl_bn_bwd_apply: dy = gamma*rstd*(g - coef0 - xhat*coef1), may alias g. */
GDL_API int gdl_bn_bwd_blocks(size_t M, int C);
GDL_API int gdl_bn_bwd_reduce(int dtype, const void* g, const void* y, const float* scale, const float* shift,
                              const float* save_mean, const float* save_rstd, int relu_mask, float* partial, size_t M,
                              int C, void* stream);
GDL_API int gdl_bn_bwd_finalize(const float* partial, int blocks, int C, double count, float* dgamma, float* dbeta,
                                float* coef, void* stream);
GDL_API int gdl_bn_bwd_apply(int dtype, const void* g, const void* y, const float* scale, const float* shift,
                             const float* save_mean, const float* save_rstd, const float* gamma, const float* coef,
                             int relu_mask, void* dy, size_t M, int C, void* stream);
/* dx = dy * (out > 0)   (may alias dy) */
GDL_API int gdl_relu_bwd(int dtype, const void* dy, const void* out, void* dx, size_t n, void* stream);
/* The fused forms the encoder engine launches by default (GDL_BN_ACC), one entry point per kernel.  They exist so that each
 * fused kernel can be tested alone (tests/test_bnacc_gpu.py); a training step reaches the same kernels through gdl_encoder_*.
 *
 * Forward statistics through integer accumulators.  A convolution's epilogue adds its tiles' per-channel sums, in fixed point,
 * to `acc`: int64 [C][2] = { round(sum y * s1), round(sum y^2 * s2) } per tile, followed by ONE flag word (int64, index 2 C) --
 * 2 C + 1 words the caller zeroes before the producer runs.  gdl_bn_acc_scales(rows): the two powers of two for a tensor of
 * `rows` = N OH OW pixels (host only; s1 = 2^(49 - L), s2 = 2^(36 - L), L = ceil(log2(rows)): exact headroom for |y| < 8192).  A
 * block whose sum does not fit its share of 2^62 (or is NaN / inf) adds nothing and sets the flag word; the consumer then
 * publishes NaN statistics.
 *   gdl_conv_fwd_acc      = gdl_conv_fwd with `acc` [K][2] + flag in place of bn_partial; split_ws / split_ws_bytes optional
 *                           (NULL: unsplit) as for gdl_conv_fwd_split -- the split-K finish kernel then adds the sums.
 *   gdl_stem_conv_fwd_acc = gdl_stem_conv_fwd likewise, acc [64][2] + flag.
 *   gdl_stem_pad_zero     = gdl_stem_pad that also clears `zero_bytes` bytes at `zero` (both multiples of 16: the engine's
 *                           accumulator arena) in the same launch.
 *   gdl_bn_act_acc        = gdl_bn_act / gdl_bn_act_bits (relu_bits optional, with relu) whose BatchNorm constants are not
 *     finalized: every block derives scale / shift of all C <= 512 channels from acc (count = rows, the tensor's M) --
 *     mean = s / rows, biased variance clamped at 0, rstd, scale = gamma rstd, shift = beta - mean scale, in double -- and block 0
 *     publishes save_mean, save_rstd, scale, shift (float32 [C], all required), updates running_mean / running_var (unbiased;
 *     optional) once and adds 1 to *nbt (optional).  Residual: res == NULL none; res alone: the raw tensor; res + res_scale /
 *     res_shift: res * res_scale + res_shift from those arrays (READ when res_acc == NULL); with res_acc (+ res_gamma, res_beta,
 *     res_save_mean, res_save_rstd required, the running pair and nbt optional) the residual BatchNorm's constants are derived
 *     and published the same way, res_scale / res_shift being written.
 *   gdl_bn_relu_maxpool_fwd_acc = gdl_bn_relu_maxpool_fwd likewise (C <= 256, count = N H W).
 * Block backward.  gdl_block_bwd_reduce: do2 = dz * (z > 0) with the reductions of bn2 (partial2) and, when yd != NULL, of the
 * downsample BatchNorm (partiald) in one pass, [gdl_bn_bwd_blocks(M, C)][C][2] = { sum do2, sum do2 * (y - mean) * rstd } each;
 * premasked != 0: dz already carries the mask, z is not read and do2 not written (both may be NULL).
 * gdl_bn_bwd_apply2: dyA = gammaA rstdA (g - coefA[0] - xhatA coefA[1]) and dyB likewise from one read of g (no ReLU mask).
 * gdl_bn_finalize_train_pair / gdl_bn_bwd_finalize_pair: gdl_bn_finalize_train / gdl_bn_bwd_finalize of two BatchNorms of
 * equal width C in one launch; tile / block counts and counts may differ, the results are those of two single launches. */
GDL_API int gdl_bn_acc_scales(size_t rows, double* s1, double* s2);
GDL_API int gdl_conv_fwd_acc(int dtype, const void* x, const void* w_krsc, void* y, int64_t* acc, const void* table, int N, int H,
                             int W, int C, int K, int R, int S, int stride, int pad, void* split_ws, size_t split_ws_bytes,
                             void* stream);
GDL_API int gdl_stem_conv_fwd_acc(int dtype, const void* xp, const void* wp, void* y, int64_t* acc, const void* table, int n_img,
                                  int H, int W, int Cin, void* stream);
GDL_API int gdl_stem_pad_zero(int dtype, const float* x, void* xp, int B, int Cin, int T, int H, int W, void* zero,
                              size_t zero_bytes, void* stream);
GDL_API int gdl_bn_act_acc(int dtype, const void* y, const int64_t* acc, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean,
                           float* save_rstd, float* scale, float* shift, const void* res, const int64_t* res_acc,
                           const float* res_gamma, const float* res_beta, float* res_running_mean, float* res_running_var,
                           int64_t* res_num_batches_tracked, float* res_save_mean, float* res_save_rstd, float* res_scale,
                           float* res_shift, size_t rows, float eps, float momentum, int relu, void* out, uint8_t* relu_bits, int C,
                           void* stream);
GDL_API int gdl_bn_relu_maxpool_fwd_acc(int dtype, const void* y, const int64_t* acc, const float* gamma, const float* beta,
                                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean,
                                        float* save_rstd, float* scale, float* shift, float eps, float momentum, void* out,
                                        uint8_t* idx, void* ymax, int N, int H, int W, int C, void* stream);
GDL_API int gdl_block_bwd_reduce(int dtype, const void* dz, const void* z, const void* y2, const void* yd, const float* mean2,
                                 const float* rstd2, const float* meand, const float* rstdd, void* do2, float* partial2,
                                 float* partiald, size_t M, int C, int premasked, void* stream);
GDL_API int gdl_bn_bwd_apply2(int dtype, const void* g, const void* yA, const float* meanA, const float* rstdA,
                              const float* gammaA, const float* coefA, void* dyA, const void* yB, const float* meanB,
                              const float* rstdB, const float* gammaB, const float* coefB, void* dyB, size_t M, int C,
                              void* stream);
GDL_API int gdl_bn_finalize_train_pair(const float* partialA, int tilesA, double countA, const float* gammaA, const float* betaA,
                                       float* running_meanA, float* running_varA, int64_t* nbtA, float* save_meanA,
                                       float* save_rstdA, float* scaleA, float* shiftA, const float* partialB, int tilesB,
                                       double countB, const float* gammaB, const float* betaB, float* running_meanB,
                                       float* running_varB, int64_t* nbtB, float* save_meanB, float* save_rstdB, float* scaleB,
                                       float* shiftB, int C, float eps, float momentum, void* stream);
GDL_API int gdl_bn_bwd_finalize_pair(const float* partialA, int blocksA, double countA, float* dgammaA, float* dbetaA,
                                     float* coefA, const float* partialB, int blocksB, double countB, float* dgammaB,
                                     float* dbetaB, float* coefB, int C, void* stream);

/* ------------------------------------------------------------------ pooling
 * nn.MaxPool2d(3,2,1): backbone.py:106, fused with the stem's BN+ReLU:
 *   out[n,p,q,c] = max over the window of relu(y*scale+shift); idx (uint8, 0..8)
 *   records the first maximum in row-major window order.
 *   ymax (optional, may be NULL) receives the RAW y at that position.
 * gdl_maxpool_bwd gathers: dx[n,h,w,c] = sum of dout over windows whose idx
 *   points at (h,w).
 * gdl_maxpool_bn_bwd_apply: the stem's backward (backbone.py:104-106 reversed) in one
 *   pass, without storing the gathered gradient g0 = maxpool_bwd(dout):
 *     dy[pos] = gamma*rstd*( (y*scale+shift > 0 ? g0 : 0) - coef0 - xhat(y)*coef1 );
 *   coef comes from gdl_bn_bwd_reduce(relu_mask=1) over the POOLED pair (dout, ymax)
 *   [sum_pos g0'*xhat(y[pos]) == sum_windows dout'*xhat(ymax)] and gdl_bn_bwd_finalize
 *   with count = N*H*W (the stem-output pixel count).
 * Global average pools of basic_model.py:73-82: x [B*T][HW][C] dtype -> feat
 *   [B][C] float32 (mean over T*HW); backward broadcasts dfeat/(T*HW). */
GDL_API int gdl_bn_relu_maxpool_fwd(int dtype, const void* y, const float* scale, const float* shift, void* out,
                                    uint8_t* idx, void* ymax, int N, int H, int W, int C, void* stream);
GDL_API int gdl_maxpool_bn_bwd_apply(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* scale,
                                     const float* shift, const float* save_mean, const float* save_rstd,
                                     const float* gamma, const float* coef, void* dy, int N, int H, int W, int C,
                                     void* stream);
GDL_API int gdl_maxpool_bwd(int dtype, const void* dout, const uint8_t* idx, void* dx, int N, int H, int W, int C,
                            void* stream);
GDL_API int gdl_avgpool_fwd(int dtype, const void* x, float* feat, int B, int T, int HW, int C, void* stream);
GDL_API int gdl_avgpool_bwd(int dtype, const float* dfeat, void* dx, int B, int T, int HW, int C, void* stream);

/* ------------------------------------------------------------------ fusion head + loss
 * ConcatFusion_DGL.forward (fusion_modules.py:51-59) and ConcatFusion.forward
 * (:38-42); nn.CrossEntropyLoss (main_dgl.py:71,102-104).  All float32.
 *   x, y: [B][512] pooled audio / visual features; W [n][1024]; b [n].
 * gdl_head_concat_fwd: out = [x,y]W^T+b, x_out = [x,0]W^T+b, y_out = [0,y]W^T+b
 *   (x_out / y_out may be NULL for the non-DGL head).
 * gdl_head_concat_bwd: autograd of the above for upstream gradients g_x_out,
 *   g_y_out, g_out (each may be NULL):
 *     dx = g_x_out W[:, :512] (+ g_out W[:, :512] if out_reaches_xy),
 *     dy = g_y_out W[:, 512:] (+ ...),
 *     dW = g_out^T [x,y] + (uni_in_dw ? g_x_out^T [x,0] + g_y_out^T [0,y] : 0), db likewise.
 *   DGL (detach + dropped head grads, main_dgl.py:110-122): out_reaches_xy = 0,
 *   uni_in_dw = 0.  Plain autograd of one backward call: uni_in_dw = 1.
 * gdl_softmax_ce: loss[0] = mean CE; dlogits = scale*(softmax-onehot)/B (may be NULL). */
GDL_API int gdl_head_concat_fwd(const float* x, const float* y, const float* W, const float* b, float* out,
                                float* x_out, float* y_out, int B, int n_classes, void* stream);
GDL_API int gdl_head_concat_bwd(const float* x, const float* y, const float* W, const float* g_x_out,
                                const float* g_y_out, const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx,
                                float* dy, float* dW, float* db, int B, int n_classes, void* stream);
/* One modality's auxiliary path of a DGL concat / sum head in ONE launch (main_dgl.py:102-122: an encoder learns from its own
 * unimodal loss only, so its backward can start as soon as ITS forward is done):
 *   u = f Wp^T + bp,  d(u) = scale*(softmax(u) - onehot(labels))/B,  df = d(u) Wp
 * f [B][512], Wp = the modality's 512 columns (row stride ldw floats: W / W + 512 with ldw 1024 for ConcatFusion_DGL,
 * fc_x / fc_y with ldw 512 for SumFusion_DGL), bp [n].  df is bit-identical to gdl_head_*_fwd + gdl_softmax_ce +
 * gdl_head_*_bwd's dx / dy with the DGL flags. */
GDL_API int gdl_head_uni_dfeat(const float* f, const float* Wp, int ldw, const float* bp, const int64_t* labels, float scale,
                               float* df, int B, int n_classes, void* stream);
/* ... for a modality whose features are `width` wide (512, 768 or 1024: the 768 Swin-T features of ConcatFusion_Swin's DGL form,
 * Wp = W + 512 with ldw = 512 + 768); df bit-identical to gdl_head_concat_xy_fwd + gdl_softmax_ce3 + gdl_head_concat_xy_bwd. */
GDL_API int gdl_head_uni_dfeat_w(const float* f, const float* Wp, int ldw, const float* bp, const int64_t* labels, float scale,
                                 float* df, int B, int n_classes, int width, void* stream);
/* The unimodal scores of OGM / OGM-GE gradient modulation (main.py:286-295, the published definitions) in ONE launch:
 *   u_a = fa Wa^T + bias_scale*ba,  u_v = fv Wv^T + bias_scale*bv      (fa, fv [B][512]; Wa, Wv: row stride ldw floats)
 *   prob[b] = {softmax(u_a[b])[labels[b]], softmax(u_v[b])[labels[b]]}   ([B][2], device)
 *   scores  = {sum_b prob[b][0], sum_b prob[b][1]}                       ([2], device; added in sample order, no float atomics)
 * ConcatFusion: Wa = W, Wv = W + 512, ldw 1024, ba = bv = fc_out.bias, bias_scale 0.5; SumFusion: fc_x / fc_y, ldw 512, their
 * biases, bias_scale 1.  n_classes <= 512.  A label outside [0, n) makes the sample's probabilities and both scores NaN.
 * `ws` (gdl_head_uni_scores_workspace_bytes, 4-byte aligned) holds a ticket counter: the caller zeroes it ONCE, every launch
 * that runs to its end leaves it zero again.  Launches sharing one `ws` must be ordered on one stream. */
GDL_API size_t gdl_head_uni_scores_workspace_bytes(void);
GDL_API int gdl_head_uni_scores(const float* fa, const float* fv, const float* Wa, const float* Wv, int ldw, const float* ba,
                                const float* bv, float bias_scale, const int64_t* labels, float* prob, float* scores, int B,
                                int n_classes, void* ws, size_t ws_bytes, void* stream);
/* The classifier of the unimodal baselines (AVClassifier_DGL with modality 'audio' / 'visual', basic_model.py:46-59, 88-122:
 * nn.Linear(512, n_classes) on the pooled features of the one encoder, trained by main.py's single CrossEntropyLoss).
 * float32: f [B][width], W [n][width], b [n]; width must be 512 and n_classes <= 512 (other sizes: GDL_ERR_ARG).
 *   gdl_head_cls_fwd: out = f W^T + b.
 *   gdl_head_cls_bwd: for an upstream gradient g_out [B][n]: df = g_out W, dW = g_out^T f, db = sum_b g_out; each of the three
 *     outputs may be NULL and is then neither computed nor touched.
 *   gdl_head_cls_ce: ONE launch for the training step -- out, loss[0] = mean CE(out, labels), dlogits = scale * (softmax(out) -
 *     onehot) / B and df = dlogits W.  out, dlogits and df are bit-identical to gdl_head_cls_fwd + gdl_softmax_ce +
 *     gdl_head_cls_bwd; loss[0] sums the B per-sample terms in one fixed order (no floating-point atomics): every output is
 *     bit-reproducible from run to run.  A label outside [0, n) gives no one-hot term and a NaN loss, as in gdl_softmax_ce.
 *     The launch keeps B floats and a counter of its own per (device, stream); the first call on a stream (and the first with a
 *     larger B) allocates them and synchronises the device, every later call is asynchronous. */
GDL_API int gdl_head_cls_fwd(const float* f, const float* W, const float* b, float* out, int B, int n_classes, int width,
                             void* stream);
GDL_API int gdl_head_cls_bwd(const float* f, const float* W, const float* g_out, float* df, float* dW, float* db, int B,
                             int n_classes, int width, void* stream);
GDL_API int gdl_head_cls_ce(const float* f, const float* W, const float* b, const int64_t* labels, float scale, float* out,
                            float* loss, float* dlogits, float* df, int B, int n_classes, int width, void* stream);
/* The junction of the step whose FUSED loss reaches the encoders, in ONE launch: the concat / sum DGL head without its .detach()
 * (the DGL ablation "no detach" and the multi-task baseline loss_f + gamma (loss_a + loss_v), main.py:177).  float32,
 * fa, fv [B][512]; Wa, Wv: row stride ldw floats; n_classes <= 512 (more: GDL_ERR_ARG, nothing is launched or touched).
 *   ConcatFusion_DGL: Wa = W, Wv = W + 512, ldw 1024, ba = bv = fc_out.bias, sum_bias 0 (the one bias serves all three sets);
 *   SumFusion_DGL:    Wa = fc_x.weight, Wv = fc_y.weight, ldw 512, their biases, sum_bias 1 (`out` carries ba + bv).
 *   out_a = fa Wa^T + ba,  out_v = fv Wv^T + bv,  out = fa Wa^T + fv Wv^T + bias                      ([B][n] each)
 *   losses[3] = {CE(out), CE(out_a), CE(out_v)}: unscaled means, as gdl_softmax_ce3 reports them
 *   g_f = (softmax(out) - onehot)/B,  g_a = scale_u (softmax(out_a) - onehot)/B,  g_v likewise          ([B][n] each)
 *   dfa = (g_a + fused_reaches g_f) Wa,  dfv = (g_v + fused_reaches g_f) Wv                            ([B][512] each)
 * The logits, the logit gradients and dfa / dfv are bit-identical to gdl_head_{concat,sum}_fwd + gdl_softmax_ce3(1, scale_u,
 * scale_u) + gdl_head_{concat,sum}_bwd(out_reaches_xy = fused_reaches)'s dx / dy.  Each loss sums its B per-sample terms in one
 * fixed order (no floating-point atomics): every output is bit-reproducible from run to run.  A label outside [0, n) gives no
 * one-hot term and NaN losses, as in gdl_softmax_ce.  The head's parameter gradients are gdl_head_{concat,sum}_bwd's, with
 * dx = dy = NULL, from g_f / g_a / g_v.
 * `ws` (gdl_head_mtl_ce_workspace_bytes(B), 4-byte aligned) holds a ticket counter and the 3 B per-sample loss terms: the caller
 * zeroes it ONCE, every launch that runs to its end leaves the counter zero again.  Launches sharing one `ws` must be ordered
 * on one stream. */
GDL_API size_t gdl_head_mtl_ce_workspace_bytes(int B);
GDL_API int gdl_head_mtl_ce(const float* fa, const float* fv, const float* Wa, const float* Wv, int ldw, const float* ba,
                            const float* bv, int sum_bias, const int64_t* labels, float scale_u, int fused_reaches, float* out,
                            float* out_a, float* out_v, float* losses, float* g_f, float* g_a, float* g_v, float* dfa, float* dfv,
                            int B, int n_classes, void* ws, size_t ws_bytes, void* stream);
/* The concat head with unequal feature widths, W [n][x_dim + y_dim] (512 audio + 768 Swin features; the reference's
 * ConcatFusion_Swin, fusion_modules.py:79-88, in its DGL form :45-59): same contract as the two calls above. */
GDL_API int gdl_head_concat_xy_fwd(const float* x, const float* y, const float* W, const float* b, float* out, float* x_out,
                                   float* y_out, int B, int n_classes, int x_dim, int y_dim, void* stream);
GDL_API int gdl_head_concat_xy_bwd(const float* x, const float* y, const float* W, const float* g_x_out, const float* g_y_out,
                                   const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx, float* dy, float* dW,
                                   float* db, int B, int n_classes, int x_dim, int y_dim, void* stream);
/* FiLM_DGL (fusion_modules.py:126-178; SURVEY next row N2): fc: Linear(512*512, 512) -- a 134 M-parameter bilinear
 * form per output, h[b][k] = u_b^T W_k v_b + bias_k -- and fc_out: Linear(512, n):
 *   out = fc_out(fc(x.detach() (x) y.detach())),  x_out = fc_out(fc(x (x) x)),  y_out = fc_out(fc(y (x) y)).
 * The outer products are never materialised; the contractions over fc.weight (537 MB) run as 1x1 convolutions /
 * weight gradients of this library in exact-f32 mode.  B <= 512 per call (the workspace grows with B: 0.47 GiB at 64,
 * 3.5 GiB at 512; gdl_head_film_workspace_bytes returns 0 beyond).  hidden: [3][B][512] float32 (h_x, h_f,
 * h_y), produced by fwd and consumed, with the SAME untouched workspace, by bwd.  bwd: any upstream gradient may
 * be NULL; dx/dy, dWfc/dbfc, dWo/dbo are optional pairs; uni_in_dw as for the other heads (0 in the DGL step). */
GDL_API size_t gdl_head_film_workspace_bytes(int B);
GDL_API int gdl_head_film_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo,
                              const float* bo, float* hidden, float* out, float* x_out, float* y_out, int B, int n_classes,
                              void* ws, size_t ws_bytes, void* stream);
GDL_API int gdl_head_film_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden,
                              const float* g_x_out, const float* g_y_out, const float* g_out, int uni_in_dw, float* dx,
                              float* dy, float* dWfc, float* dbfc, float* dWo, float* dbo, int B, int n_classes, void* ws,
                              size_t ws_bytes, void* stream);
/* FiLM trained jointly (fusion_modules.py:91-124 at dim = 512; BASELINE config 1 with the FiLM head): nothing is detached and
 * only the fused form exists,
 *   h_f[b][k] = sum_ij x_b[i] y_b[j] W[k,i,j] + bias_k,   out = fc_out(h_f)        (replaces :116-122: two unsqueezes, bmm,
 *   view, two Linears).
 * T[(k,i)][b] = (W_k y_b)[i] is computed for the y columns only (B rounded up to 64 columns, against 2 * roundup(B, 32) of
 * gdl_head_film_fwd: half the f32 contraction over fc.weight at B = 64).  Backward from g_out [B][n] (autograd of the above):
 *   dh = g_out Wo;   dx[b][i] = sum_k dh[b][k] T[(k,i)][b]  (no GEMM: T is still in the workspace);
 *   dy[b][j] = sum_(k,i) dh[b][k] x_b[i] W[k,i,j]  (one weight-gradient contraction over fc.weight);
 *   dWfc[k,i,j] = sum_b dh[b][k] x_b[i] y_b[j], dbfc = sum_b dh;  dWo = g_out^T h_f, dbo = sum_b g_out.
 * hidden: [B][512] float32 (h_f alone -- NOT gdl_head_film_fwd's [3][B][512]), produced by joint_fwd and consumed, with the
 * SAME untouched workspace, by joint_bwd.  Workspace: gdl_head_film_workspace_bytes(B); B <= 512 and the error codes as for
 * gdl_head_film_fwd / _bwd.  dx/dy, dWfc/dbfc, dWo/dbo are optional pairs.  `out` is bit-identical to gdl_head_film_fwd's. */
GDL_API int gdl_head_film_joint_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo,
                                    const float* bo, float* hidden, float* out, int B, int n_classes, void* ws,
                                    size_t ws_bytes, void* stream);
GDL_API int gdl_head_film_joint_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden,
                                    const float* g_out, float* dx, float* dy, float* dWfc, float* dbfc, float* dWo, float* dbo,
                                    int B, int n_classes, void* ws, size_t ws_bytes, void* stream);
/* GatedFusion_DGL (fusion_modules.py:213-250, x_gate = True; SURVEY next row N2): fc_x, fc_y: Linear(512, 512),
 * fc_out: Linear(512, n).  hx = fc_x(x), hy = fc_y(y) ([B][512], returned: saved for the backward);
 *   out = fc_out(sigmoid(hx.detach()) * hy.detach()),  x_out = fc_out(sigmoid(hx) * hx),  y_out = fc_out(sigmoid(hy) * hy).
 * Backward for upstream gradients on (x_out, y_out, out), any may be NULL: dx, dy (through fc_x / fc_y; `out` never
 * reaches them), dWo / dbo = out's contribution (+ the unimodal ones if uni_in_dw), optionally dW1, db1, dW2, db2
 * (NULL in the DGL step, whose script drops them and whose loss_f does not reach fc_x / fc_y).  ws: 2*B*512 floats. */
GDL_API int gdl_head_gated_fwd(const float* x, const float* y, const float* W1, const float* b1, const float* W2,
                               const float* b2, const float* Wo, const float* bo, float* hx, float* hy, float* out,
                               float* x_out, float* y_out, int B, int n_classes, void* stream);
GDL_API int gdl_head_gated_bwd(const float* x, const float* y, const float* hx, const float* hy, const float* W1,
                               const float* W2, const float* Wo, const float* g_x_out, const float* g_y_out,
                               const float* g_out, int uni_in_dw, float* dx, float* dy, float* dW1, float* db1, float* dW2,
                               float* db2, float* dWo, float* dbo, float* ws, int B, int n_classes, void* stream);
/* GatedFusion trained jointly (fusion_modules.py:181-210; BASELINE config 1 with the gated head): hx = fc_x(x), hy = fc_y(y),
 *   x_gate != 0: out = fc_out(sigmoid(hx) * hy)          (:203-205)
 *   x_gate == 0: out = fc_out(hx * sigmoid(hy))          (:206-208)
 * hx, hy [B][512] are returned (saved for the backward).  With x_gate != 0 `out` is bit-identical to gdl_head_gated_fwd's.
 * Backward from g_out [B][n], autograd of the above (gate = hx, value = hy if x_gate, else swapped; s = sigmoid(gate)):
 *   dm = g_out Wo;   d(value) = dm * s;   d(gate) = dm * value * s (1 - s);
 *   dx = dhx W1, dy = dhy W2;   dW1 = dhx^T x, db1 = sum_b dhx;   dW2 = dhy^T y, db2 = sum_b dhy;
 *   dWo = g_out^T (s * value), dbo = sum_b g_out.
 * dx/dy, dW1/db1/dW2/db2, dWo/dbo are optional groups.  ws: 2*B*512 floats. */
GDL_API int gdl_head_gated_joint_fwd(const float* x, const float* y, const float* W1, const float* b1, const float* W2,
                                     const float* b2, const float* Wo, const float* bo, float* hx, float* hy, float* out,
                                     int x_gate, int B, int n_classes, void* stream);
GDL_API int gdl_head_gated_joint_bwd(const float* x, const float* y, const float* hx, const float* hy, const float* W1,
                                     const float* W2, const float* Wo, const float* g_out, int x_gate, float* dx, float* dy,
                                     float* dW1, float* db1, float* dW2, float* db2, float* dWo, float* dbo, float* ws, int B,
                                     int n_classes, void* stream);
/* SumFusion_DGL (fusion_modules.py:16-30; SURVEY next row N2): fc_x, fc_y: Linear(512, n).
 *   x_out = fc_x(x), y_out = fc_y(y), out = fc_x(x.detach()) + fc_y(y.detach()).
 * Same flag meaning as the concat head; the sum head has two weight matrices [n][512] and two biases
 * (dbx = sum_b (g_out + uni*g_x_out), dby likewise).
 * SumFusion trained jointly (fusion_modules.py:5-13: out = fc_x(x) + fc_y(y), one loss) is the same pair of calls:
 * fwd with x_out = y_out = NULL, bwd with g_x_out = g_y_out = NULL, out_reaches_xy = 1, uni_in_dw = 0. */
GDL_API int gdl_head_sum_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy,
                             const float* by, float* out, float* x_out, float* y_out, int B, int n_classes, void* stream);
GDL_API int gdl_head_sum_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* g_x_out,
                             const float* g_y_out, const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx,
                             float* dy, float* dWx, float* dbx, float* dWy, float* dby, int B, int n_classes, void* stream);
/* the three losses of the DGL step (loss_f, loss_a, loss_v; main_dgl.py:102-104) in one launch: losses[k] and dlogits_k
 * as gdl_softmax_ce would leave them for (logits_k, scale_k); any dlogits_k may be NULL */
GDL_API int gdl_softmax_ce3(const float* logits0, const float* logits1, const float* logits2, const int64_t* labels,
                            float scale0, float scale1, float scale2, float* losses, float* dlogits0, float* dlogits1,
                            float* dlogits2, int B, int n_classes, void* stream);
GDL_API int gdl_softmax_ce(const float* logits, const int64_t* labels, float scale, float* loss, float* dlogits, int B,
                           int n_classes, void* stream);
/* valid() (main_dgl.py:185-222) without its per-sample host loop: per-class counters (int64[n_classes] each, the
 * caller zeroes them once and accumulates over the batches of the validation set):
 *   num[label[i]] += 1;  acc[label[i]] += (argmax(out[i]) == label[i]);  likewise acc_a / acc_v from out_a / out_v
 * (first maximum wins, like np.argmax; softmax is monotone so it is not evaluated).  out_a/acc_a and out_v/acc_v
 * may be NULL together.  Accuracies are sum(acc)/sum(num) etc. as in main_dgl.py:222. */
GDL_API int gdl_eval_count(const float* out, const float* out_a, const float* out_v, const int64_t* labels, int B,
                           int n_classes, int64_t* num, int64_t* acc, int64_t* acc_a, int64_t* acc_v, void* stream);

/* ------------------------------------------------------------------ input pipeline
 * The device-side stages of the datasets' __getitem__:
 *   gdl_logspec: clip to [-1, 1], librosa.stft(n_fft, hop_length) with librosa's defaults (periodic Hann window of
 *     n_fft samples, center=True), log(|X| + 1e-7)  (dataset/CramedDataset.py:62-66: n_fft 512, hop 353;
 *     KSDataset.py:144-149 / VGGSoundDataset.py:117-122: 256 / 128).  wave: float32 [B][n_samples] (already resampled
 *     and tiled / cropped to its fixed length by the host; gdl_wave_logspec below does the staging too); out: float32 [B][n_fft/2+1][gdl_logspec_frames()], the
 *     tensor the DataLoader yields.  pad_mode: how the n_fft/2 samples either side are made up -- librosa >= 0.10
 *     pads with zeros (GDL_PAD_CONSTANT), older releases reflect (GDL_PAD_REFLECT); the reference does not pin a version.
 *   gdl_wave_logspec: what the datasets do between the decoded file and that spectrogram, and the spectrogram, in one launch:
 *     the decode scale of 16-bit PCM (x / 32768, soundfile's float read), librosa.load's mono=True mix-down (np.mean over the
 *     channels: (l + r) / 2), the tiling (np.tile(samples, 3) of CREMA-D / AVE, the `while len / rate < 10: tile(., 2)` of the
 *     16 kHz datasets), the window [start, start + n_samples), the clip to [-1, 1], gdl_logspec's transform, and, where a
 *     dataset has it, np.resize(spectrogram, (out_h, out_w))  (KSDataset.py:139-149, VGGSoundDataset.py:112-122,
 *     Kinect400.py:120-129, Audioset.py:140-153, CramedDataset.py:60-66 / 155-163, AVEDataset.py:81-88).  Both tilings are the
 *     periodic extension of the clip, staged[p] = mono[(start + p) mod len], 0 <= p < n_samples, as long as the window ends
 *     inside the tiled length `limit`; the padding of the STFT (zeros or reflection) is applied to that staged window.
 *     src: the decoded clips packed in one device buffer of src_bytes bytes (4-byte aligned, every clip starting on a 4-byte
 *     boundary), each float32 (GDL_WAVE_F32) or int16 (GDL_WAVE_S16), one or two channels interleaved as files store them.
 *     desc: int64 [B][6] in device memory (8-byte aligned),
 *       { byte offset of the clip in src, len (samples per channel), channels, format, start, limit }.
 *     out_h = out_w = 0: out is float32 [B][n_fft/2+1][gdl_logspec_frames(n_samples, hop)], bit-identical to gdl_logspec of
 *     the staged window (the two kernels share the transform's device code).  Otherwise out is float32 [B][out_h][out_w]
 *     under np.resize's rule, a flat re-layout and not an interpolation: out.flat[i] = spec.flat[i mod (bins * frames)].
 *     wave_out: NULL, or float32 [B][n_samples] that receives the staged, clipped window.
 *     Resampling is not done here: a clip is at the rate its dataset works at (the 16 kHz datasets' files are; CREMA-D and
 *     AVE clips are resampled to 22050 Hz by the host and passed as float32).
 *     A sample whose clip does not lie inside src (or starts off a 4-byte boundary), or with len < 1 or >= 2^31, channels not
 *     1 or 2, an unknown format, start < 0 or not start + n_samples <= limit < 2^31, is written as NaN -- its out and its
 *     wave_out row -- and nothing of it is read.  Limits: B <= 65535, n_samples < 2^31 - 4096, out_h * out_w < 2^31.
 *   gdl_frames_normalize: transforms.ToTensor() + Normalize(mean, std) (CramedDataset.py:77-81): uint8 [n_img][H][W][3]
 *     -> float32 [n_img][3][H][W], ((x / 255) - mean[c]) / std[c]; mean / std: 3 host floats each.
 *   gdl_frames_resized_crop: the datasets' whole visual transform in one launch -- training: RandomResizedCrop(size),
 *     RandomHorizontalFlip(), ToTensor(), Normalize(mean, std); evaluation: Resize((size, size)), ToTensor(), Normalize
 *     (CramedDataset.py:76-88) -- for boxes and flips the caller has drawn on the host.
 *     src: n_img decoded frames packed in one uint8 device buffer of src_bytes bytes (4-byte aligned), each HWC with
 *     3 channels and a row pitch of 3 * width; frames may differ in size.  desc: int64 [n_img][8] in device memory,
 *       { byte offset of the frame in src, height, width, box top, box left, box height, box width, flip (0 / 1) };
 *     the whole frame as the box is Resize.  Image n is frame t = n % T of sample b = n / T; out: float32
 *     [B][3][T][out_h][out_w] (the datasets' permute(1, 0, 2, 3) is folded into the store; T = 1: [n_img][3][out_h][out_w]).
 *     Arithmetic: the box is cropped first, so pixels outside it never contribute; then Pillow's ImagingResample with
 *     the bilinear filter, which is what Resize runs on a PIL image: separable, the horizontal pass first, then the
 *     vertical, the intermediate image rounded to uint8.  Per output index i of a pass in -> out: scale = in / out,
 *     filterscale = support = max(1, scale), center = (i + 0.5) * scale, taps x from max(0, int(center - support + 0.5))
 *     up to min(in, int(center + support + 0.5)), weight triangle((x - center + 0.5) / filterscale), the weights
 *     normalised to sum 1 in double precision and rounded to 22 fractional bits, k = int(0.5 + w * 2^22);
 *     result = clip((2^21 + sum k[x] * pixel[x]) >> 22, 0, 255) in int32.  Then out[.., w] = resized[.., flip ? out_w-1-w : w],
 *     ((x / 255) - mean[c]) / std[c] as gdl_frames_normalize.  The result is bit-identical to that recipe
 *     (tests/resize_ref.py restates it in NumPy); against torch's antialiased uint8 CPU resize it differs by at most one grey level
 *     on about 1 % of the pixels (docs/parity_log.md).
 *     Limits: frames and boxes up to 65535 a side; a box must pass gdl_frames_resized_crop_box_ok(box_h, box_w, out_h,
 *     out_w) (1 = fits): the kernel keeps the coefficient tables, one source row of the box and the rows of one output
 *     row's vertical taps in 40 KB of LDS -- for a 224 x 224 output a 1080 x 1920 box fits, 16:9 boxes up to about 2200
 *     columns wide do, a 2160 x 3840 box does not.  The caller checks boxes (it has them on the host; gdl.data does); the kernel clamps a box into its frame,
 *     and an image whose frame does not lie inside src or whose box does not fit is written as NaN, never read out of bounds. */
#define GDL_PAD_CONSTANT 0
#define GDL_PAD_REFLECT 1
GDL_API int gdl_logspec_frames(int n_samples, int hop);
GDL_API int gdl_logspec(const float* wave, int B, int n_samples, int n_fft, int hop, int pad_mode, float* out, void* stream);
#define GDL_WAVE_F32 0
#define GDL_WAVE_S16 1
GDL_API int gdl_wave_logspec(const void* src, size_t src_bytes, const int64_t* desc, int B, int n_samples, int n_fft, int hop,
                             int pad_mode, int out_h, int out_w, float* wave_out, float* out, void* stream);
GDL_API int gdl_frames_normalize(const uint8_t* frames, int64_t n_img, int H, int W, const float* mean, const float* std,
                                 float* out, void* stream);
GDL_API int gdl_frames_resized_crop_box_ok(int box_h, int box_w, int out_h, int out_w);
GDL_API int gdl_frames_resized_crop(const uint8_t* src, size_t src_bytes, const int64_t* desc, int n_img, int B, int T, int out_h,
                                    int out_w, const float* mean, const float* std, float* out, void* stream);

/* ------------------------------------------------------------------ the epoch planner of the device-resident loader
 * What the reference's DataLoader and datasets draw per sample -- the shuffled order (DataLoader(shuffle=True)), the window start
 * (random.randint, KSDataset.py:139-149), RandomResizedCrop's box and RandomHorizontalFlip's coin per frame
 * (CramedDataset.py:76-88) -- computed on the device for a whole epoch in ONE launch, as the descriptor tables the two stage
 * kernels above read.  Nothing is drawn, checked or copied by the host; a value is a function of (seed, epoch, sample index).
 * gdl_loader_plan fills the tables of `count` consecutive epoch positions first .. first + count - 1.
 *   In (int64 device memory, 8-byte aligned): clips [N][5] = { byte offset, len, channels, format, limit } -- the first four
 *   are columns 0..3 of gdl_wave_logspec's rows, limit the tiled length; frames [N][T][3] = { byte offset, H, W }; labels [N].
 *   Scalars: N in [1, 2^31 - 1], T in [1, 64], seed, epoch, first, count, shuffle and augment (0 / 1), n_samples and start_high
 *   (the window's length and its largest start: start_high + n_samples < 2^31), out_h x out_w (the resize's output size, which
 *   must fit that kernel's tables).  draw: seven HOST doubles { scale_lo, scale_hi, ratio_lo, ratio_hi, log(ratio_lo),
 *   log(ratio_hi), p_flip }; the caller takes the logarithms so that the device and a restatement use the same constants.
 *   Out (int64 device memory): index [count], label [count], wave_desc [count][6] in gdl_wave_logspec's row format, crop_desc
 *   [count * T][8] in gdl_frames_resized_crop's row format, frame t of position p at row p * T + t.  Batch k of size B is then
 *   gdl_wave_logspec(.., wave_desc + 6 B k, B, ..) and gdl_frames_resized_crop(.., crop_desc + 8 B T k, B T, B, T, ..).
 *   first < 0, count < 1, first + count > N or a limit above: GDL_ERR_ARG, nothing launched, nothing written.
 * Arithmetic (all integers exact; tests/loader_ref.py restates it on NumPy):
 *   words(c0, purpose, t, k) = philox4x32_10(counter (c0, 0xC0000000 | purpose << 24 | t << 8 | k, epoch low, epoch high),
 *   key (seed low, seed high)); purposes PERM 0, BOX 1, FLIP 2, WAVE 3.  Bits 31 and 30 of counter word 1 are set together only
 *   here (gdl_optim_modulate: word 1 < 2^29; gdl_dul_sample: 0x80000000 | modality), so the three users of one seed stay disjoint.
 *   u(w) = (w + 0.5) 2^-32.  Every draw is keyed by the sample's index, never by its position: a sample's window, boxes and flips
 *   in an epoch do not depend on the batch size or the rank layout.
 *   position -> index: shuffle = 0: the position.  shuffle = 1: a keyed bijection of [0, N) evaluated per element, nothing
 *   stored or sorted -- a balanced Feistel network on 2 kb bits, kb = max(1, ceil(bit_length(N - 1) / 2)), mask = 2^kb - 1: from
 *   L = v >> kb, R = v & mask, six rounds (L, R) <- (R, L ^ (words(R, PERM, 0, round)[0] & mask)), v' = L << kb | R; repeated
 *   from v' while v' >= N (cycle walking; the domain is below 4 N, so fewer than 4 passes on average).  N = 1 gives 0.
 *   window start = (words(index, WAVE, 0, 0)[0] * (start_high + 1)) >> 32, a 64-bit product; drawn with augment = 0 as well (the
 *   reference draws it in test mode too).  wave_desc row = { offset, len, channels, format, start, limit }.
 *   frame t, augment = 1: torchvision's published RandomResizedCrop.get_params in double.  Try k = 0 .. 9, w = words(index, BOX,
 *   t, k): a = (H W) (scale_lo + (scale_hi - scale_lo) u(w[0])), r = exp(log_ratio_lo + (log_ratio_hi - log_ratio_lo) u(w[1])),
 *   bw = rint(sqrt(a r)), bh = rint(sqrt(a / r)) (ties to even, Python's round), no operation fused; accepted if 0 < bw <= W and
 *   0 < bh <= H, then top = (w[2] (H - bh + 1)) >> 32, left = (w[3] (W - bw + 1)) >> 32.  No try accepted: W / H < ratio_lo:
 *   bw = W, bh = rint(W / ratio_lo); W / H > ratio_hi: bh = H, bw = rint(H ratio_hi); otherwise the whole frame; a side that
 *   rounds to 0 is 1; top = (H - bh) div 2, left = (W - bw) div 2.  flip = u(words(index, FLIP, t, 0)[0]) < p_flip.
 *   frame t, augment = 0: the whole frame, no flip (Resize).  A frame with a side outside [1, 65535] gets the whole-frame row in
 *   either mode; gdl_frames_resized_crop writes such an image as NaN.
 * Departures from the reference, all in which random stream is read, none in a distribution's shape: Philox instead of Python's
 *   and torch's Mersenne streams; the range reduction (w n) >> 32 instead of rejection sampling, biased by less than n / 2^32
 *   (random.randint(0, 80000): 2e-5); a keyed bijection instead of torch.randperm.
 * The LDS limit of the resize kernel: gdl_frames_resized_crop_box_ok fails only if a side exceeds 65535 or if the tables plus one
 *   staged row plus one output row's taps exceed 40 KB, and every term of that sum grows with the box's sides (tap counts, the
 *   staged row, the taps' rows); so if the whole frame passes, every box inside it passes.  The planner therefore does not test
 *   boxes: the owner of the dataset tests each distinct frame size once (gdl.DeviceDataset does), and the stage kernel's own
 *   guard (NaN) stays as the backstop. */
GDL_API int gdl_loader_plan(const int64_t* clips, const int64_t* frames, const int64_t* labels, int64_t N, int T, uint64_t seed,
                            int64_t epoch, int64_t first, int64_t count, int shuffle, int augment, int64_t n_samples,
                            int64_t start_high, int out_h, int out_w, const double* draw, int64_t* index, int64_t* label,
                            int64_t* wave_desc, int64_t* crop_desc, void* stream);

/* ------------------------------------------------------------------ clip + grad stats + SGD
 * clip_grad_norm_(params, 40, 2) (main_dgl.py:129), the logged
 * sum_p mean|grad_p| per encoder (:132-143) and optim.SGD(momentum, weight_decay)
 * (:249,154) over FLAT float32 arenas.  seg_offsets[nseg+1] (int64, element
 * offsets, host memory) delimit the parameters; seg_group[nseg] (int32, host) is
 * 0 = fusion head, 1 = audio_net, 2 = visual_net.
 * gdl_optim_grad_stats writes stats[0..3] = {total_norm (pre-clip), clip_coef,
 *   audio_grad_sum, visual_grad_sum (both post-clip)} on the device.
 * gdl_optim_sgd_step: g *= clip_coef*grad_scale (written back); d = g + wd*p;
 *   m = mu*m + d; p -= lr*m  (momentum arena starts at zero, which reproduces
 *   torch's first-step `buf = d`).
 * gdl_optim_adamw_step: optim.AdamW(lr, betas=(beta1, beta2), eps, weight_decay) as main_dgl.py:255-256 builds it for
 *   `--optimizer Adam` (torch's _single_tensor_adam, decoupled weight decay, no amsgrad), in torch's order:
 *   g *= clip_coef*grad_scale (written back); p *= 1 - lr*wd; m += (1 - beta1)*(g - m); v = beta2*v + (1 - beta2)*g*g;
 *   p -= lr/(1 - beta1^step) * m / (sqrt(v)/sqrt(1 - beta2^step) + eps).  Both moment arenas start at zero.
 * gdl_optim_adagrad_step: optim.Adagrad(lr, eps, weight_decay) as main_dgl.py:252-253 builds it for `--optimizer AdaGrad`
 *   (lr_decay 0): g *= clip_coef*grad_scale (written back); d = g + wd*p (not written back); s += d*d;
 *   p -= lr * d / (sqrt(s) + eps).  The accumulator arena starts at zero (torch's initial_accumulator_value).
 *   Both: `step` counts the updates, the first is 1 (step < 1 is an error); the bias corrections are derived from it, and
 *   every per-step scalar from the double hyperparameters, in double on the host, then rounded to float once.  One launch
 *   over the whole arena, no host sync; the clipped gradient is written back only where clip_coef*grad_scale != 1.
 * The object owns no device memory: gdl_optim_create only builds host tables; `ws` (gdl_optim_workspace_bytes, 16-byte
 * aligned, caller-owned) holds the descriptor tables in its head -- uploaded, ordered on `stream`, the first time
 * gdl_optim_grad_stats is called with that pointer -- and the per-chunk partial sums behind them.  Keep the workspace intact
 * between calls (or pass another pointer: the tables are uploaded again).  gdl_optim_bind_workspace (round 4) uploads the tables
 * unconditionally: call it whenever the workspace memory may have changed hands without its ADDRESS changing (a caching
 * allocator returns a freed block at the same address; another kernel scribbled over it), and before capturing
 * gdl_optim_grad_stats into a HIP graph -- the implicit first-use upload is a pageable-memory copy, which a capture refuses. */
typedef struct gdl_optim gdl_optim_t;
GDL_API int gdl_optim_create(gdl_optim_t** out, const int64_t* seg_offsets, const int32_t* seg_group, int nseg);
GDL_API void gdl_optim_destroy(gdl_optim_t* o);
GDL_API size_t gdl_optim_workspace_bytes(const gdl_optim_t* o);
GDL_API int gdl_optim_grad_stats(gdl_optim_t* o, const float* grads, float max_norm, float grad_scale, float* stats,
                                 void* ws, size_t ws_bytes, void* stream);
GDL_API int gdl_optim_bind_workspace(gdl_optim_t* o, void* ws, size_t ws_bytes, void* stream);
GDL_API int gdl_optim_stats_len(const gdl_optim_t* o); /* 4 + 2*nseg floats */
GDL_API int gdl_optim_sgd_step(gdl_optim_t* o, float* params, float* grads, float* momentum, const float* stats,
                               float grad_scale, float lr, float mu, float wd, void* stream);
GDL_API int gdl_optim_adamw_step(gdl_optim_t* o, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                 const float* stats, float grad_scale, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int64_t step, void* stream);
GDL_API int gdl_optim_adagrad_step(gdl_optim_t* o, float* params, float* grads, float* state_sum, const float* stats,
                                   float grad_scale, double lr, double eps, double weight_decay, int64_t step, void* stream);
/* OGM / OGM-GE gradient modulation (main.py:286-330), between gdl_optim_grad_stats and the update, over the gradient arena in
 * place.  seg_mark[nseg] (int32, host): 0 = untouched, 1 = audio-modulated, 2 = visual-modulated (the 4-D tensors of the two
 * encoders); a marked segment has at least 2 elements.  With k = clip_coef*grad_scale (stats[1] of the statistics pass that
 * ran on `ws` just before) and `scores` = {score_a, score_v} on the device (gdl_head_uni_scores):
 *   ratio_v = score_v/score_a;  ratio_v > 1: coeff_v = 1 - tanh(alpha*ratio_v), coeff_a = 1;
 *                               otherwise:   coeff_a = 1 - tanh(alpha/ratio_v), coeff_v = 1
 *   marked segment of modality m:  g <- (g*k)*coeff_m                  (noise = 0: OGM)
 *                                  g <- (g*k)*coeff_m + sigma*z        (noise = 1: OGM_GE; BOTH modalities get the noise)
 *     sigma = k*std(g) + 1e-8, std the unbiased standard deviation of the whole tensor (in double from the statistics pass's
 *     sum of squares and a sum pass of this call);  z ~ N(0, 1) from Philox4x32-10, key = (seed low, seed high 32 bits),
 *     counter = (i >> 2, 0, step, 0) for arena element i, which takes normal i & 3 of the Box-Muller pairs of words (0, 1)
 *     and (2, 3), u(w) = ((w >> 8) + 0.5) * 2^-24, r = sqrt(-2 ln u(w0)), theta = 2 pi u(w1): a function of (seed, step, i)
 *     alone -- not of the launch geometry, the rank or the segment table.
 *   unmarked segment:  g <- g*k, as the update kernels store it.
 * Call the update that follows with stats = NULL and grad_scale = 1.  Everything stays on the device, nothing synchronises.
 * mod_stats (gdl_optim_modulate_stats_len = 8 + nseg floats, device): {score_a, score_v, ratio_v, coeff_a, coeff_v, 0, 0, 0,
 * sigma of every segment (0 where unmarked or noise = 0)}.  `mod_ws` (gdl_optim_modulate_workspace_bytes, 16-byte aligned,
 * caller-owned) is separate from `ws`, whose size does not change; gdl_optim_modulate_bind uploads the marks into it (ordered on
 * `stream`) and must have been called with the same pointer. */
GDL_API size_t gdl_optim_modulate_workspace_bytes(const gdl_optim_t* o);
GDL_API int gdl_optim_modulate_stats_len(const gdl_optim_t* o);
GDL_API int gdl_optim_modulate_bind(gdl_optim_t* o, const int32_t* seg_mark, void* mod_ws, size_t mod_ws_bytes, void* stream);
GDL_API int gdl_optim_modulate(gdl_optim_t* o, float* grads, const float* stats, float grad_scale, const float* scores,
                               float alpha, int noise, int64_t seed, int64_t step, float* mod_stats, const void* ws,
                               void* mod_ws, void* stream);

/* ------------------------------------------------------------------ probabilistic-embedding branch (--pe, --beta)
 * main.py's `--pe 1 --beta b`: behind an encoder's final map x [n_img][P][512] (the last block's output after its ReLU, M = n_img
 * P rows, row r of sample b = r / (T P)) two stacks Conv2d(512, 512, 1) + BatchNorm2d(512), `mu_dul_backbone` and
 * `logvar_dul_backbone` (models/swin_transformer.py:574-582; the scripts ran them on the ResNet), the reparameterised sample and
 * its pool (:643-667, basic_model.py:73-82) and the KL term `regurize` (main.py:92-102), which joins the loss as
 * beta (reg_a + reg_v) (main.py:191-213).  float32 arithmetic whatever the storage dtype of the maps.
 *
 * Training forward.  z_mu = x W_mu^T + b_mu, z_lv = x W_lv^T + b_lv (gdl_conv_fwd_bias), each stack's train-mode BatchNorm over
 * the M rows (gdl_bn_stats, gdl_bn_finalize_train: biased variance, eps 1e-5, running statistics with momentum 0.1 and the
 * unbiased variance; the bias is part of the batch mean that reaches running_mean).  A stack's constants travel as
 * bn = float [4][512] = {scale, shift, save_mean, save_rstd}.  gdl_dul_sample:
 *     mu = fmaf(z_mu, scale_mu, shift_mu)   lv = fmaf(z_lv, scale_lv, shift_lv)   sd = expf(0.5f lv)   out = fmaf(eps, sd, mu)
 *     f[b][c] = (sum of out[r][c] over the sample's T P rows) / (T P)
 *     reg[0]  = (sum over rows and channels of 0.5f (sd^2 + mu^2 - logf(sd^2 + 1e-8f) - 1)) / n_img
 *   (n_img, not B: `regurize` takes the mean over dim 0 of the [B T, ...] maps).  mu_map / sd_map / eps_map / out_map: optional
 *   float32 [M][512] copies (NULL in a training step) -- what main.py's model returned as a_mul / a_std.
 *   One launch; the pool and the KL sum each have one fixed order (dul.hip states them), no floating-point atomic: two launches
 *   on the same data give the same bits.  `ws`: gdl_dul_sample_workspace_bytes, 256-byte aligned, zeroed ONCE by the caller
 *   (it holds the ticket counter of ticket.h, handed back at zero), one per stream.
 * Noise.  eps_in != NULL: the caller's float32 [M][512] map, used bit for bit.  eps_in == NULL: standard normals of the
 *   modulation's generator (Philox4x32-10, Box-Muller with the radius through a double logarithm) keyed
 *     counter = (e >> 2, 0x80000000 | modality, step low, step high), key = (seed low, seed high)
 *   for element e = r 512 + c, which takes normal e & 3 of the Box-Muller pairs of words (0, 1) and (2, 3): a function of
 *   (seed, step, modality, e) alone.  Word 1 of a modulation counter is below 2^29, so the ranges are disjoint, and audio and
 *   visual differ in word 1.  The noise is never stored: the backward entries regenerate it from the same arguments.
 * Backward from the head's df [B][512], k = beta / n_img, g = df[b][c] / (T P):
 *     d_mu = g + k mu      d_sd = g eps + k (sd - sd / (sd^2 + 1e-8f))      d_lv = d_sd 0.5f sd
 *   gdl_dul_bwd_reduce -> partial_mu, partial_lv [blocks][512][2] = per-block {sum d, sum d xhat} of each stack, blocks =
 *   gdl_bn_bwd_blocks(M, 512), xhat = (z - save_mean) save_rstd; gdl_bn_bwd_finalize (count = M) of each -> dgamma, dbeta, coef;
 *   gdl_dul_bwd_apply -> dz = gamma save_rstd (d - coef0 - xhat coef1) of both stacks, in `dtype`.  Then dx = dz_mu W_mu +
 *   dz_lv W_lv (gdl_conv_dgrad, the second with the first as its addend) is the gradient w.r.t. the post-ReLU map (it reaches
 *   the engine as gdl_encoder_backward's dfmap_nchw, through gdl_nhwc_to_nchw_f32), dW = dz^T x
 *   (gdl_conv_wgrad), and db_conv = 0 exactly -- a named departure: a bias in front of a train-mode BatchNorm has a
 *   mathematically zero gradient, torch leaves the rounding noise of sum dz there.
 *   beta = 0 is allowed (k = 0: the KL terms vanish from the gradient, reg is still reported).  Non-finite values propagate
 *   as torch's do (a huge lv gives sd = inf).
 * Eval.  out = mu with running statistics, then the pool; pooling commutes with a 1x1 convolution and a per-channel affine, so
 *   gdl_dul_eval: out[b][k] = fmaf(dot(w_mu[k], f[b]) + b_mu[k], scale[k], shift[k]) on the engine's pooled f [B][512], w_mu
 *   float32 [512][512], scale / shift from gdl_bn_finalize_eval; each dot product in one fixed order; out must not alias f.
 *   The logvar stack is not evaluated.  A named departure from the literal order (convolve every position, then pool), exact
 *   in real arithmetic.
 * All entries: C must be 512, n_img a multiple of T, P, T, n_img >= 1, n_img P < 2^25; maps, bn, coef, df and partials 16-byte
 * aligned (gamma_*, w_mu, b_mu -- views of a parameter arena -- 4-byte); GDL_ERR_ARG with a message and no launch otherwise. */
GDL_API size_t gdl_dul_sample_workspace_bytes(int dtype, int n_img, int T);
GDL_API int gdl_dul_sample(int dtype, const void* z_mu, const void* z_lv, const float* bn_mu, const float* bn_lv,
                           const float* eps_in, int64_t seed, int64_t step, int modality, float* f, float* reg, float* mu_map,
                           float* sd_map, float* eps_map, float* out_map, int n_img, int T, int P, int C, void* ws,
                           size_t ws_bytes, void* stream);
GDL_API int gdl_dul_bwd_reduce(int dtype, const void* z_mu, const void* z_lv, const float* df, const float* eps_in, int64_t seed,
                               int64_t step, int modality, float beta, const float* bn_mu, const float* bn_lv, float* partial_mu,
                               float* partial_lv, int n_img, int T, int P, int C, void* stream);
GDL_API int gdl_dul_bwd_apply(int dtype, const void* z_mu, const void* z_lv, const float* df, const float* eps_in, int64_t seed,
                              int64_t step, int modality, float beta, const float* bn_mu, const float* bn_lv,
                              const float* gamma_mu, const float* gamma_lv, const float* coef_mu, const float* coef_lv, void* dz_mu,
                              void* dz_lv, int n_img, int T, int P, int C, void* stream);
GDL_API int gdl_dul_eval(const float* f, const float* w_mu, const float* b_mu, const float* scale, const float* shift, float* out,
                         int B, int C, void* stream);

/* ------------------------------------------------------------------ ResNet18 encoder engine
 * `resnet18(modality, args)` / ResNet.forward (backbone.py:75-201, 255-257) plus the
 * pooling glue of AVClassifier_DGL.forward (basic_model.py:73-82), as one planned
 * sequence of the kernels above on one stream.
 *
 * Parameter order everywhere below = named_parameters() order of the reference
 * module (60 tensors): conv1.weight, bn1.weight, bn1.bias, then per BasicBlock
 * conv1.weight, bn1.{weight,bias}, conv2.weight, bn2.{weight,bias}
 * [, downsample.0.weight, downsample.1.{weight,bias}].  BatchNorm buffer order =
 * the 20 BatchNorm layers in the same traversal.
 */
typedef struct gdl_encoder gdl_encoder_t;
#define GDL_ENC_NPARAMS 60
#define GDL_ENC_NBN 20
GDL_API int gdl_encoder_create(gdl_encoder_t** out, int modality, int dtype, int B, int T, int H, int W);
GDL_API void gdl_encoder_destroy(gdl_encoder_t* e);
/* enable != 0: gdl_encoder_backward forks the weight gradients (which are off the dy -> dx dependency chain)
 * onto an engine-owned side stream and joins it back into the caller's stream before returning control of
 * that stream, so the call keeps its single-stream semantics.  Off by default.  Measured on MI355X: a whole
 * step slows down 1.15-1.4x once more than FOUR streams carry work, or when a stream has a non-default
 * priority, so a caller running {main, audio, visual} streams enables this for the visual engine only (the
 * critical path) and not at all when a collective's stream is active as well. */
GDL_API int gdl_encoder_side_stream(gdl_encoder_t* e, int enable);
/* The same fork / join onto a stream of the CALLER's (NULL = the null stream) instead of an engine-owned one: no new
 * hardware queue.  Meant for a stream the caller already has and that idles during the step -- DGLTrainer hands the audio
 * engine the stream `step()` was called on, which only orders the step before and behind (round 4: 5.63 -> 5.43 ms per
 * step; the audio chain, a quarter of the work in ~100 small launches, had been the last to finish).  The engine enqueues
 * on that stream only inside gdl_encoder_backward(_phase) (between a wait for the engine's stream and an event the
 * engine's stream waits for), so work the caller puts there before / after the call is ordered as on one stream.  May be
 * called again with another stream; gdl_encoder_side_stream(e, 0) returns to none. */
GDL_API int gdl_encoder_borrow_side_stream(gdl_encoder_t* e, void* stream);
GDL_API size_t gdl_encoder_workspace_bytes(const gdl_encoder_t* e);
GDL_API int gdl_encoder_param_numel(const gdl_encoder_t* e, int64_t* numel /*[60]*/);
GDL_API int gdl_encoder_out_shape(const gdl_encoder_t* e, int* n_img, int* h, int* w);
/* bind the caller-owned workspace (device) and the parameter / gradient / buffer tables (host arrays of device ptrs) */
GDL_API int gdl_encoder_bind(gdl_encoder_t* e, void* workspace, size_t bytes);
GDL_API int gdl_encoder_set_params(gdl_encoder_t* e, const float* const* params, float* const* running_mean,
                                   float* const* running_var, int64_t* const* num_batches_tracked);
/* forward.  x: the reference's input tensor, float32 [B][Cin][T][H][W] contiguous.
 * training != 0: batch statistics, running-stat update, activations kept for backward.
 * feat_out: [B][512] float32 pooled features (may be NULL); fmap_nchw: [B*T][512][h][w]
 * float32, the tensor ResNet.forward returns (may be NULL). */
GDL_API int gdl_encoder_forward(gdl_encoder_t* e, const float* x, int training, float* feat_out, float* fmap_nchw,
                                void* stream);
/* backward of the last training forward.  Exactly one of dfeat ([B][512]) / dfmap_nchw
 * is non-NULL.  grads: 60 device pointers (float32, reference layouts), overwritten.
 * The call may be repeated for one forward, with another upstream gradient and other `grads`: it reads the activations the
 * forward kept and writes only the engine's gradient scratch and `grads`, so every call returns what the first call after that
 * forward would have returned for its arguments (DGLTrainer's pareto step: two backwards of one forward, in stream order). */
GDL_API int gdl_encoder_backward(gdl_encoder_t* e, const float* dfeat, const float* dfmap_nchw, float* const* grads,
                                 void* stream);
/* The same backward in two calls, for data-parallel callers: phase 1 = the upstream gradient and layer4 -- when it
 * returns (in stream order) the last 15 gradient tensors, 8.4 M of the 11.2 M parameters, are final and their
 * all-reduce can overlap phase 2 (layer3 .. layer1 and the stem).  Phase 2 takes no dfeat / dfmap (pass NULL). */
GDL_API int gdl_encoder_backward_phase(gdl_encoder_t* e, int phase, const float* dfeat, const float* dfmap_nchw,
                                       float* const* grads, void* stream);
/* serial number of the last training forward (to detect stale activations) */
GDL_API int64_t gdl_encoder_forward_serial(const gdl_encoder_t* e);
/* Round 4: the training forward's BatchNorm statistics travel through 64-bit fixed-point accumulators with finite headroom
 * (mean |y| of a block's rows < 8192 / channel tiles).  A BatchNorm whose sums exceeded it -- or were NaN / inf -- gets NaN
 * statistics instead of wrapped integers; since ReLU turns NaN into 0 the activations may not show it, so this returns the number
 * of such BatchNorms in the last training forward (0 = fine; < 0 = -error code).  Synchronises `stream`.  A diverged
 * nn.BatchNorm2d of the reference shows as inf / NaN in its outputs (backbone.py:45-48,104,144); here ask this. */
GDL_API int gdl_encoder_bn_overflow(gdl_encoder_t* e, void* stream);

/* ------------------------------------------------------------------ feature-diversity monitor
 * main.py's get_feature_diversity (:77-89), which its training loop applies to each encoder's final feature map at every step
 * (:183-184), averages over the epoch (:339-340, :356) and prints as "Audio similar / Visual similar" (:657, :662).  Per image,
 * with x_p the C = 512 channels at position p (P = h w positions):
 *   c_p = x_p - mean_C(x_p),  s_p = sqrt(sum_C c_p^2 / (C - 1)),  R_pq = (c_p . c_q) / (s_p s_q),  d = ||R||_F / P^2
 * per_image[i] = d of image i (n_img floats, may be NULL), mean_out[0] = their mean.  accum (2 floats, may be NULL):
 * accum[0] += mean_out[0], accum[1] += 1 -- an epoch's sum and count, written by the launch itself in stream order, so a whole
 * epoch needs no host sync.  All arithmetic is float32 whatever the storage type (a bf16 map is widened; the centred values are
 * never rounded); the mean sums the n_img terms in one fixed order (no floating-point atomics): every output is bit-reproducible
 * from run to run.  A position whose 512 channels are all equal has s_p = 0: NaN for that image and for the mean, as the
 * script's 0 / 0 gives.
 *   layout GDL_LAYOUT_NHWC: map [n_img][P][C] of `dtype` (float32 or bf16; the engine's activations), 16-byte aligned;
 *   layout GDL_LAYOUT_NCHW: map [n_img][C][P] float32 (the tensor the drop-in modules return), 4-byte aligned.
 * `ws` (gdl_feature_diversity_workspace_bytes(n_img), 256-byte aligned, so that the counter's line holds nothing else): a ticket
 * counter on a 256-byte line of its own and n_img floats; the caller zeroes it ONCE, every launch that runs to its end leaves
 * the counter zero again (the engine's call, gdl_encoder_feature_diversity, asks the same of its `ws`).  Launches sharing one
 * `ws` must be ordered on one stream.  GDL_ERR_ARG, with a message and without a launch: C != 512, P outside [1, 256],
 * n_img < 1, a null map / mean_out / ws, a short ws, bf16 with NCHW, a misaligned pointer. */
#define GDL_LAYOUT_NHWC 0
#define GDL_LAYOUT_NCHW 1
GDL_API size_t gdl_feature_diversity_workspace_bytes(int n_img);
GDL_API int gdl_feature_diversity(const void* map, int dtype, int layout, int n_img, int P, int C, float* per_image,
                                  float* mean_out, float* accum, void* ws, size_t ws_bytes, void* stream);
/* The same on the final map of the engine's last forward, training or eval (the last block's output, n_img x h w x 512 in the
 * engine's storage type; n_img, h, w: gdl_encoder_out_shape).  GDL_ERR_STATE before any forward.  Launch it on the stream that
 * ran the forward: stream order is what protects the buffer.  Nothing but the next gdl_encoder_forward writes it -- the
 * backward only reads it (the last block's ReLU mask and BatchNorm reductions), on the caller's stream, and the side lane's
 * weight gradients read the blocks' inputs and never this map -- so the call may stand in front of the backward, behind it,
 * or beside it on another stream that has waited for the forward, as long as it is ordered before the next forward. */
GDL_API int gdl_encoder_feature_diversity(gdl_encoder_t* e, float* per_image, float* mean_out, float* accum, void* ws,
                                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ step journal
 * The scripts' per-step log kept on the device.  main_dgl.py appends [audio_grad_sum, visual_grad_sum] to a CSV at every step
 * (:132-152), adds loss_f / loss_a / loss_v `.item()` into Python floats whose sums over len(dataloader) are its epoch line
 * (:156-165), and prints the losses with torch.abs(out_a).mean() / torch.abs(out_v).mean() every 100 steps (:125-127, :144-146);
 * main.py adds the two diversity sums (:339-340) and OGM's `ratio v / coefficient v / coefficient a` (:308-312).  Each of these
 * is a host sync per step there.  gdl_journal_append writes them as ONE row of GDL_JOURNAL_COLS floats per step into a ring in
 * the caller's device buffer and adds the row to the epoch's sums beside it: a whole epoch needs no host sync and one host copy.
 * Columns of a row:
 *    0-2   loss_f, loss_a, loss_v            `losses` (n_losses = 3), or losses[0] in all three (n_losses = 1: the unimodal
 *                                            model returns `out, out, out`)
 *    3-6   total_norm, clip_coef, audio_grad_sum, visual_grad_sum      gdl_optim_grad_stats' stats[0..3]
 *    7-8   mean |out_a|, mean |out_v|        over n_logits = B n values each (main_dgl.py:146); either pointer may be NULL
 *    9-10  a_diversity, v_diversity          one float each (gdl_feature_diversity's mean_out), may be NULL
 *   11-15  score_a, score_v, ratio_v, coeff_a, coeff_v                 gdl_optim_modulate's mod_stats[0..4], may be NULL
 * Columns 0-6 and 9-15 are copies of the source floats, bit for bit; a NULL source writes NaN into its columns.  Columns 7-8:
 * float32, one fixed order -- thread t of the one 256-thread block adds |x[t]|, |x[t + 256]|, ... in turn, a butterfly folds
 * each wave, the four wave sums are added as (w0 + w1) + (w2 + w3), one division by (float)n_logits; no floating-point atomic,
 * so two launches on the same data give the same bits, and (all terms being non-negative) the relative error against the
 * exact mean of the same values is at most (ceil(n_logits / 256) + 8 + 1) 2^-24 for n_logits < 2^24.
 * The buffer (gdl_journal_bytes(capacity) bytes, 16-byte aligned), header, then accumulators, then rows:
 *   byte   0  int64  count: rows appended since the header was last zeroed;  byte 8: three reserved int64
 *   byte  32  double acc[12]: acc[c] += (double)row[c] for c = 0..10 at every append, in step order -- the script's
 *             `_loss += x.item()` exactly, so acc[c] / count is its epoch mean over ALL `count` steps whether or not the ring has
 *             wrapped; a NaN propagates as it does there; acc[11] is unused
 *   byte 128  float  rows[capacity][GDL_JOURNAL_COLS]: the append writes row count % capacity, then count becomes count + 1 --
 *             the ring keeps the newest `capacity` rows
 * Zero the first 128 bytes (hipMemsetAsync, ordered on the stream) before the first append and to start a new epoch; the rows
 * need no clearing.  No host-side state enters the launch -- the cursor lives in the buffer -- so every step's call has the
 * same arguments and may be captured into a graph.  One launch of one work-group; appends to one buffer must be ordered on one
 * stream, behind whatever writes the sources.  GDL_ERR_ARG, with a message and without a launch: journal NULL or not 16-byte
 * aligned, capacity < 1, n_losses not 1 or 3, losses or stats NULL, n_logits < 0, a non-NULL out_a / out_v with n_logits = 0.
 * gdl_journal_bytes: 128 + 64 capacity; 0 for capacity < 1. */
#define GDL_JOURNAL_COLS 16
GDL_API size_t gdl_journal_bytes(int64_t capacity);
GDL_API int gdl_journal_append(void* journal, int64_t capacity, const float* losses, int n_losses, const float* stats,
                               const float* out_a, const float* out_v, int64_t n_logits, const float* div_a, const float* div_v,
                               const float* ogm, void* stream);

/* ------------------------------------------------------------------ evaluation report: the score bank
 * What the papers' tables give beyond valid()'s three accuracies -- mAP, top-k, the confusion matrices of the fused / audio /
 * visual logit sets -- computed on the device: one launch per batch behind gdl_eval_count, one launch pair and ONE host copy at
 * the end.  Not a port of a reference script (its valid() stops at the accuracies).  All state lives in one caller-owned
 * device buffer of gdl_eval_bank_bytes(n_classes, capacity, sets) bytes, 16-byte aligned; n_classes <= 512, sets = 1 (the fused
 * set alone) or 3 (fused, audio, visual), capacity = samples it can hold (< 2^31).  The caller keeps the append offset.
 *   byte 0             int64  skipped              samples whose label lies outside [0, n)
 *   byte 8             int64  nonfinite[3]         per set: rows holding a NaN / inf logit (samples with a valid label only)
 *   byte 32            int64  num[n]               samples per class (valid labels)
 *   + 8 n              int64  rank_hist[sets][n]   [s][r]: samples whose label has rank r in set s; top-k = sum over r < k
 *   + 8 sets n         int64  confusion[sets][n][n]  row = label, column = prediction
 *   ---- gdl_eval_bank_reset_bytes(n, sets) = 32 + 8 n (1 + sets + sets n): everything above.  Zero it (hipMemsetAsync on the
 *        stream) before the first append and for a new report; nothing below needs clearing.
 *   then               double ap[sets][n]          gdl_eval_bank_ap's result; NaN for a class without a positive
 *   then               double mAP[3], 8 bytes of padding
 *   then (16-aligned)  int32  labels[capacity]     -1 for a skipped sample; the array is rounded up to 16 bytes
 *   then               float  probs[sets][n][capacity]   class-major: one class's scores over all samples are contiguous
 * gdl_eval_bank_append -- rows offset .. offset + B - 1 from out / out_a / out_v [B, n] and int64 labels[B], one launch, per
 * sample and set: the float32 softmax (row maximum; expf(l - max); their sum in ascending class order; lse = max + logf(sum);
 * p = expf(l - lse)) stored transposed into probs; the prediction (first maximum of the logits, strict >, as gdl_eval_count);
 * the label's rank  #{j : l_j > l_lab} + #{j < lab : l_j == l_lab}  (rank 0 is the event prediction == label);
 * rank_hist[s][rank] += 1, confusion[s][label][prediction] += 1, num[label] += 1 (64-bit integer atomics: order-free; there is
 * no floating-point atomic).  A label outside [0, n), range-checked at 64 bits: labels[row] = -1, skipped += 1, NaN in the
 * row's probs, nothing else.  A row with a non-finite logit: nonfinite[s] += 1, NaN in that set's probs of the row, and no
 * rank_hist / confusion entry and no part in the average precision of that set.
 * gdl_eval_bank_ap -- over the first N rows, per class c and set s, scikit-learn's average_precision_score (step-wise, ties
 * grouped) on the stored float32 probabilities, without a sort:
 *     ap[s][c] = (1 / |pos_c|) sum_{i in pos_c}  #{j : label_j = c, p_jc >= p_ic} / #{j : p_jc >= p_ic}
 * j over the samples with a valid label and a finite row in set s.  Probabilities are compared by their bit patterns as
 * unsigned integers (they are non-negative: the float order, whatever the denormal mode); both counts are exact integers, each
 * quotient one float64 division, the quotients added in ascending sample order, one division by |pos_c|: within
 * (|pos_c| + 2) 2^-53 of the exact rational value.  A class without a positive gives NaN (scikit-learn: 0.0 and a warning).
 * mAP[s] = the float64 mean of the non-NaN classes in class order (NaN if there is none).  No block waits for another and
 * nothing is accumulated across blocks: two calls give identical bytes.
 * Calls on one bank must be ordered on one stream, behind whatever writes the logits.  GDL_ERR_ARG, with a message and without
 * a launch: bank NULL or not 16-byte aligned; n_classes outside [1, 512]; sets not 1 or 3; capacity outside [1, 2^31);
 * bank_bytes below gdl_eval_bank_bytes; out or labels NULL; out_a / out_v given with sets = 1 or missing with sets = 3; B < 1;
 * offset < 0 or offset + B > capacity; N outside [0, capacity].  gdl_eval_bank_bytes / gdl_eval_bank_reset_bytes: 0 for such
 * a shape. */
GDL_API size_t gdl_eval_bank_bytes(int n_classes, int64_t capacity, int sets);
GDL_API size_t gdl_eval_bank_reset_bytes(int n_classes, int sets);
GDL_API int gdl_eval_bank_append(void* bank, size_t bank_bytes, int n_classes, int64_t capacity, int sets, const float* out,
                                 const float* out_a, const float* out_v, const int64_t* labels, int B, int64_t offset,
                                 void* stream);
GDL_API int gdl_eval_bank_ap(void* bank, size_t bank_bytes, int n_classes, int64_t capacity, int sets, int64_t N, void* stream);

/* ------------------------------------------------------------------ linear probe of a frozen encoder
 * One epoch of the linear probe's fit: main.py's unimodal step with the encoder removed, on features that are already on the
 * device.  bank [N][512] float32 (the pooled features of an eval-mode encoder), labels [N] int64, order [steps][B] int32 (device):
 * step s trains on the rows order[s][0 .. B-1].  Per step
 *   out = f W^T + b;  loss = mean CE(out, y);  clip_grad_norm_({dW, db}, max_norm);  SGD(lr, momentum, weight_decay)
 * with the logits and the softmax of gdl_head_cls_ce (the same device functions), the gradient sums in sample order, and the
 * clip and the update of gdl_optim_grad_stats / gdl_optim_sgd_step: the norm accumulated in double, coef = min(1, max_norm /
 * (norm + 1e-6)), d = coef g + wd p, m = mu m + d, p -= lr m.  W [n][512], b [n] and their momentum buffers mW, mb (zero before
 * the first epoch) are updated in place; loss_acc[0] += the sum of the steps' mean losses (each a float, widened), loss_acc[1] +=
 * steps -- the caller zeroes the two doubles where an epoch's mean should start.
 * The loop over the steps runs inside the call: three launches per step, ordered by the stream alone -- no block waits for
 * another, no floating-point atomic, every sum in one fixed order: two calls from the same state and order table give the same
 * bits.  Nothing is allocated and nothing synchronises.  `ws` (gdl_linprobe_workspace_bytes, 16-byte aligned) is scratch: it
 * holds no counter and needs no zeroing; calls sharing one `ws` must be ordered on one stream.
 * A label outside [0, n) gives no one-hot term and a NaN loss, as in gdl_softmax_ce.  An order index outside [0, N) never reads
 * outside the bank: the step uses row 0 in its place and its loss is NaN (check the table on the host: gdl.LinearProbe does).
 * GDL_ERR_ARG, with a message and without a launch or a write: n_classes outside [1, 512], B < 1, steps < 0, N < 1, a NULL
 * pointer (order may be NULL with steps = 0), W / mW / ws not 16-byte aligned; GDL_ERR_WORKSPACE: ws_bytes too small.
 * B need not divide N.  gdl_linprobe_workspace_bytes: 0 for arguments the epoch would refuse. */
GDL_API size_t gdl_linprobe_workspace_bytes(int B, int n_classes);
GDL_API int gdl_linprobe_epoch(const float* bank, const int64_t* labels, int64_t N, const int32_t* order, int steps, int B,
                               float* W, float* b, float* mW, float* mb, int n_classes, float lr, float momentum,
                               float weight_decay, float max_norm, double* loss_acc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ prototypical modal rebalance (PMR) on the joint step
 * A prototype cross-entropy on each encoder's pooled feature, added to the joint loss for the modality that is behind (Fan et
 * al., CVPR 2023; DESIGN.md section 8 is this project's statement of the arithmetic).  All tensors float32 on the device, feature
 * width 512, at most 512 classes.  No launch has a floating-point atomic, no block waits for another, every sum has one order:
 * two calls on the same inputs give the same bytes.  Nothing is allocated, nothing synchronises, there is no workspace.
 *
 * gdl_proto_ce -- one modality: f [B][512] features, P [n][512] prototypes, labels [B] int64.
 *   d[b][j] = sqrt(sum_k (f[b][k] - P[j][k])^2): per lane the differences of features l, l + 64, .. squared and added as one fmaf
 *   chain, then the xor butterfly 32 .. 1 (a direct sum, not the |f|^2 - 2 f.P + |P|^2 expansion), one sqrtf;  sim = -d;
 *   softmax as in gdl_softmax_ce: row max, expf, the exponentials summed in ascending class order, lse = max + logf(sum),
 *   p = expf(sim - lse);  q[b][j] = ((p[b][j] - [j == label_b]) / B) / d[b][j], 0 where d = 0 (torch's sqrt backward: NaN);
 *   u[b][k] = sum_j q[b][j] (P[j][k] - f[b][k]), classes ascending, one fmaf chain = d lossp / d f[b][k] of
 *   lossp = CrossEntropyLoss(sim, labels) (mean over B).
 *   Writes u [B][512]; terms [2][B]: terms[b] = p[b][label_b], terms[B + b] = lse_b - sim[b][label_b]; and sim [B][n] unless sim
 *   is NULL.  A label outside [0, n): no one-hot term, terms[b] = 0, terms[B + b] = NaN.
 *   GDL_ERR_ARG, without a launch: width != 512, n_classes outside [1, 512], B < 1, a NULL pointer other than sim.
 * gdl_proto_apply -- both modalities, behind the two gdl_proto_ce on a stream that orders them: folds terms_a / terms_v
 *   ([2][B] each) into score_a, score_v and the two loss sums, each in the order of the loss sums of gdl_softmax_ce (256 partial
 *   sums p[b & 255] taking b, b + 256, .. in turn, then the tree p[i] += p[i + o], o = 128 .. 1), then
 *     rho = score_a / score_v;  rho > 1: beta = 0, lam = alpha;  rho < 1: beta = alpha, lam = 0;  otherwise (1 or NaN) both 0
 *     dfa[b][k] = fmaf(beta, u_a[b][k], dfa[b][k]);  dfv[b][k] = fmaf(lam, u_v[b][k], dfv[b][k])
 *   A side whose coefficient is 0 is neither read nor written: its df keeps its bits.  stats[8] = {score_a, score_v, rho, beta,
 *   lam, lossp_a, lossp_v, 0} with lossp = (loss sum) / B.
 *   GDL_ERR_ARG: width != 512, B outside [1, 2^22], a NULL pointer, u_a / u_v / dfa / dfv not 16-byte aligned.
 * gdl_proto_update -- one feature bank: bank [N][512], labels [N] int64, P [n][512] updated in place.  Per class c the rows with
 *   label c are added in ascending row order into float64 accumulators (one block walks the whole bank for its class: the row range
 *   is not split, so there are no partial sums to combine), mean = sum / count in float64, then
 *     first != 0: P_c = mean;   first == 0: P_c = (1 - momentum) P_c + momentum mean       (float64, rounded to float32 once)
 *   A class without a row keeps its prototype (the published script divides by zero there).  count[n] int64 = rows per class;
 *   info[2] int64 = {classes without a row, rows whose label is outside [0, n): they belong to no class}.
 *   GDL_ERR_ARG: width != 512, n_classes outside [1, 512], N < 1, momentum outside [0, 1], a NULL pointer. */
GDL_API int gdl_proto_ce(const float* f, const float* P, const int64_t* labels, float* u, float* terms, float* sim, int B,
                         int n_classes, int width, void* stream);
GDL_API int gdl_proto_apply(const float* terms_a, const float* terms_v, const float* u_a, const float* u_v, float* dfa, float* dfv,
                            float alpha, float* stats, int B, int width, void* stream);
GDL_API int gdl_proto_update(const float* bank, const int64_t* labels, int64_t N, float* P, int n_classes, int width,
                             double momentum, int first, int64_t* count, int64_t* info, void* stream);

/* ------------------------------------------------------------------ alternating unimodal training on a shared head (MLA)
 * The device arithmetic of gdl.MLATrainer (Zhang et al., CVPR 2024; DESIGN.md section 8 is this project's statement of the
 * method): the projector P [512][512] that shapes the shared head's weight gradient, and the entropy-weighted fusion of the two
 * unimodal logit sets at test time.  All tensors float32 on the device.  No launch has a floating-point atomic, no block waits
 * for another, every sum has one order that does not depend on the launch geometry: two calls on the same inputs give the same
 * bytes.  Nothing is allocated, nothing synchronises.  dot512(x, y) below is ONE order: 64 partial sums, partial l taking
 * x[l + 64 m] y[l + 64 m] for m = 0 .. 7 as one fmaf chain from 0, then the tree s[l] += s[l ^ o], o = 32 .. 1.
 *
 * gdl_mla_feature_mean -- r[k] = (sum_b h[b][k]) / B for h [B][512]: plain adds from 0 with b ascending, one division.
 *   GDL_ERR_ARG: B < 1, a NULL pointer.
 * gdl_mla_projector_update -- P updated in place against r [512] and the host scalar alpha > 0:
 *     k[i] = dot512(P[i], r);   c = alpha + dot512(r, k);   P[i][j] = P[i][j] - (k[i] k[j]) / c
 *   the product rounded first, then one division, then one subtraction, none contracted: a P that is symmetric stays symmetric
 *   bit for bit.  normalize != 0: P = P / ||P||_F afterwards, with ||P||_F = (float)sqrt(S), S the double sum of the 512 row sums
 *   dot512(P[i], P[i]) (float) -- partial l taking rows l + 64 m, m ascending, then the same tree -- and one division per entry.
 *   Two launches, three with normalize (k lives in the workspace between them: no block reads a row another block rewrites).
 *   ws: gdl_mla_projector_workspace_bytes() bytes, 4-byte aligned, contents irrelevant.
 *   GDL_ERR_ARG, without a launch: a NULL pointer, alpha not a finite positive number, a workspace too small or misaligned.
 * gdl_mla_project -- dW [n][512] <- dW P^T in place: new dW[c][i] = dot512(old dW[c], P[i]).  A block owns whole rows of dW and
 *   has loaded them before it stores.  GDL_ERR_ARG, nothing launched or touched: n_classes outside [1, 512], a NULL pointer.
 * gdl_mla_fuse -- out_a, out_v [B][n] -> out [B][n] and, unless lam is NULL, lam [B][2] = {lam_a, lam_v}.  Per sample and set:
 *     lse = max + logf(sum_j expf(l_j - max)), the exponentials added in ascending class order;  p_j = expf(l_j - lse);
 *     e = sum_j p_j (lse - l_j) in ascending class order (every term >= 0: a p_j of 0 contributes 0);
 *   w_m = expf(-(e_m - min(e_a, e_v))), lam_m = w_m / (w_a + w_v), out = lam_a out_a + lam_v out_v (two rounded products and one
 *   add).  Equal entropies give lam = 0.5, 0.5 exactly.  A NaN or inf logit in either set makes both lam and the whole out row
 *   NaN.  dynamic == 0: lam = 0.5, 0.5, no entropy is computed (a non-finite logit then reaches only its own class of out).
 *   GDL_ERR_ARG: n_classes outside [1, 512], B < 1, a NULL pointer other than lam. */
GDL_API int gdl_mla_feature_mean(const float* h, int B, float* r, void* stream);
GDL_API size_t gdl_mla_projector_workspace_bytes(void);
GDL_API int gdl_mla_projector_update(float* P, const float* r, float alpha, int normalize, void* ws, size_t ws_bytes,
                                     void* stream);
GDL_API int gdl_mla_project(float* dW, const float* P, int n_classes, void* stream);
GDL_API int gdl_mla_fuse(const float* out_a, const float* out_v, int B, int n_classes, int dynamic, float* out, float* lam,
                         void* stream);

/* ------------------------------------------------------------------ MMPareto gradient integration on the multi-task step
 * One encoder's gradient of the fused loss, g_m, and of its own (weighted) unimodal loss, g_u -- n float32 each, the encoder's
 * tensors as ONE vector -- become one gradient, written over g_m (Wei & Hu, ICML 2024; DESIGN.md section 8 is this project's
 * statement of the arithmetic).  Where the two agree the result is the min-norm point of the segment [g_u, g_m], rescaled to the
 * norm of the plain sum; where they conflict it is the plain sum.  g_m, g_u and info need 4-byte alignment only (ranges of a
 * flat gradient arena).  ONE call = two launches on `stream`, nothing is allocated, nothing synchronises, no device value is
 * read back:
 *   1. S_mm = sum g_m^2, S_uu = sum g_u^2, S_mu = sum g_m g_u: every product formed in double, the sums kept in double and added
 *      in ONE order that depends on n alone -- blocks of 8192 elements, within a block 256 sums (sum t takes the elements
 *      4 (t + 256 k) .. + 3, k = 0 .. 7, in ascending order) folded by the tree p[i] += p[i + o], o = 128 .. 1; then the blocks'
 *      sums, sum t taking blocks t, t + 256, .., and the same tree.  No floating-point atomic, no block waits for another; the grid,
 *      the stream and the alignment of the pointers do not enter: the same values give the same bytes wherever they lie.
 *   2. by every block of the second launch, from those sums, in double:
 *        S_mu > 0 and all three sums finite ("agreement", branch 1):
 *            D = S_mm - 2 S_mu + S_uu;   gamma = D > 0 ? clamp((S_uu - S_mu) / D, 0, 1) : 0.5;   w_m = 2 gamma, w_u = 2 (1 - gamma)
 *            N_h^2 = w_m^2 S_mm + 2 w_m w_u S_mu + w_u^2 S_uu;   N_s^2 = S_mm + 2 S_mu + S_uu
 *            s = N_h^2 > 0 and finite ? sqrt(N_s^2 / N_h^2) : 1                                   (>= 1 up to rounding)
 *        otherwise ("sum", branch 0):  gamma = 0.5, w_m = w_u = 1, s = 1
 *        c_m = (float)(scale s w_m),  c_u = (float)(scale s w_u);    g_m[i] = fmaf(c_u, g_u[i], c_m * g_m[i])  (the product rounded)
 *      A NaN or inf anywhere in g_m or g_u therefore gives the plain sum scaled by `scale`, with the NaN where it was.
 * info[8] (device) = {S_mm, S_uu, S_mu (rounded to float), gamma, w_m, w_u, s, branch}.  ws: gdl_pareto_workspace_bytes(n) bytes,
 * 16-byte aligned, contents irrelevant before the call; behind it its first two floats are {c_m, c_u} as the combine used them.
 * g_u is not written.  Calls sharing one `ws` must be ordered on one stream.
 * GDL_ERR_ARG, with a message and without a launch or a write: n outside [1, 2^36], a NULL pointer, a misaligned pointer, a
 * workspace too small.  gdl_pareto_workspace_bytes(n <= 0) = 0. */
GDL_API size_t gdl_pareto_workspace_bytes(int64_t n);
GDL_API int gdl_pareto_integrate(float* g_m, const float* g_u, int64_t n, float scale, float* info /* [8], device */, void* ws,
                                 size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ measurement tap
 * Optional HIP-event timing of every kernel launch (off by default).  While enabled, each
 * launcher records an event pair on the launching stream and its algorithmic work (flops for
 * the MFMA-bound conv kernels, bytes for the HBM-bound ones).  gdl_prof_collect synchronises
 * the device and returns per-slot totals: launches[s], ms[s], work[s], s < gdl_prof_nslots().
 * gdl_prof_slot_bound: 1 = MFMA-bound (work in flops), 0 = HBM-bound (work in bytes). */
GDL_API int gdl_prof_enable(int on);
GDL_API int gdl_prof_enabled(void); /* 1 while the tap records (callers that replay captured graphs run eagerly then) */
/* tuning aid: in a -DGDL_TIMING build the conv kernels write per-block s_memtime stamps to buf[block][8]
 * (uint64); in the normal build this returns GDL_ERR_ARG */
GDL_API int gdl_debug_timing_buffer(void* buf);
/* record only launches of the kernel with this name (NULL or "" = all kernels) */
GDL_API int gdl_prof_set_filter(const char* name);
GDL_API int gdl_prof_nslots(void);
GDL_API const char* gdl_prof_slot_name(int slot);
GDL_API int gdl_prof_slot_bound(int slot);
GDL_API int gdl_prof_collect(int64_t* launches, double* ms, double* work);
/* Combined roofline (round 4; measurement only): the convolution launchers also state their algorithmic HBM bytes (operands once
 * + result).  After gdl_prof_collect, floor_ms[s] = the sum over slot s's launches of max(flop / peak_flops, bytes / peak_bytes)
 * -- what the launches would take at the peaks, each priced against the roof that binds it -- and bytes[s] their algorithmic
 * bytes (either pointer may be NULL).  gdl_prof_set_peaks: the two peaks (defaults: 2.5e15 flop/s bf16 MFMA, 8e12 B/s HBM3E). */
GDL_API int gdl_prof_set_peaks(double peak_flops, double peak_bytes);
GDL_API int gdl_prof_collect_floor(double* floor_ms, double* bytes);
/* Utilisation timeline (round 5; measurement only, tools/utilisation_timeline.py): the records the tap holds, in enqueue order,
 * one per launch -- slot[i], lane[i] (the launching stream, numbered in order of first appearance), start_ms[i] / end_ms[i]
 * relative to the earliest start among them (HIP events: the kernel's own begin / end for the hipExtLaunchKernelGGL taps),
 * work[i] (flops or bytes as gdl_prof_slot_bound says) and bytes[i] (algorithmic HBM bytes of an MFMA-bound launch, 0 = not
 * stated).  Call it BEFORE gdl_prof_collect (which clears the records).  Synchronises the device.  Returns the number of
 * records held (at most `cap` are written; any pointer may be NULL), < 0 = -error code. */
GDL_API int gdl_prof_timeline(int cap, int32_t* slot, int32_t* lane, double* start_ms, double* end_ms, double* work, double* bytes);

/* ---------------------------------------------------------------------------------------------------------------------
 * Swin visual encoder (/root/reference/models/swin_transformer.py, which the DGL script does not
 * reach -- main_dgl.py:236-240 -- so the Swin + DGL-head model is a new composition).  Tokens are rows [N*L][ld] of
 * `dtype`, ld = channels rounded up to a multiple of 64, padding columns zero.  Every nn.Linear (qkv, proj, fc1, fc2,
 * PatchMerging.reduction) and the 4x4/4 PatchEmbed convolution is a 1x1 gdl_conv_fwd / gdl_conv_dgrad / gdl_conv_wgrad on
 * zero-padded weights (gdl_swin_pack_matrix); the entry points below are everything else.  Vectors (bias, gamma, beta)
 * are float32 in the padded layout.
 *   gdl_swin_patch_gather   frames [B,3,T,H,W] f32 -> GEMM rows [B*T*(H/p)*(W/p)][64], columns (c,kh,kw)  (:463,:480)
 *   gdl_swin_bias_act       mode 0: y += b;  1: u = y + b, y = gelu(u);  2: y = y + b + res               (:26-42,:287-290)
 *   gdl_swin_drop_path      DropPath of a residual branch (timm.models.layers.drop_path, scale_by_keep; :218,:290,:293):
 *                           out = (res ? res : 0) + scale[row / L] * y, scale[frame] = 0 or 1 / keep_prob (drawn by the caller:
 *                           the reference draws them from torch's generator); forward with res, backward without; out may be y
 *   gdl_swin_ln_fwd / _bwd  nn.LayerNorm(eps 1e-5) over the C real channels; stats [M][2] = (mean, rstd); the backward
 *                           adds `add` (the residual branch's gradient) and returns [2][ld] = (d gamma, d beta)
 *   gdl_swin_colsum         db[ld] = column sums of g; with u != NULL first g <- g * gelu'(u) (in place)
 *   gdl_swin_attn_fwd/_bwd  WindowAttention incl. cyclic shift, mask and relative-position bias (:124-157,:222-285) on
 *                           QKV rows [q | k | v] (three ld-wide segments, head h at h*32); the backward returns dqkv and
 *                           d(relative_position_bias_table) [(2w-1)^2][heads]
 *   gdl_swin_merge          PatchMerging's 2x2 concatenation [N,H,W,C] -> [N,H/2,W/2,4C] (:336-344) / its adjoint
 *   gdl_swin_token_mean     AdaptiveAvgPool2d((1,1)) over the L tokens (:629-631) -> float32 [N][C], and its backward
 *   gdl_swin_pack_matrix    float32 [n][k] -> `dtype` [np][kp] (+ transposed [kp][np]), rows / columns in segments of
 *                           nseg / kseg stored at pitch nseg_pad / kseg_pad (QKV rows: 3 x 96 -> 3 x 128)
 *   gdl_swin_unpack_matrix  float32 padded [np][kp] -> float32 real [n][k] (weight gradients back to parameter shape)
 * ------------------------------------------------------------------------------------------------------------------- */
GDL_API int gdl_swin_patch_gather(int dtype, const float* x, void* a, int B, int T, int H, int W, int patch, void* stream);
/* Both gradients of y[M][N] = x[M][K] W^T (nn.Linear; swin_transformer.py:26-42 Mlp.fc1, :78-157 qkv) from ONE pass over dy:
 * dx[M][K] = dy . W (bf16) and dW[N][K] = dy^T . x (float32), for the shapes gdl_linear_bwd_ok accepts (bf16, K = 128, N = 384,
 * M >= 16384: stage 1 of Swin-T) -- what gdl_conv_dgrad + gdl_conv_wgrad (R = S = 1) compute in two passes over dy.  wT: the
 * weight as [K][N] (the layout gdl_swin_pack_matrix's dstT / gdl_conv_dgrad take).  ws: gdl_linear_bwd_workspace_bytes.
 * Kreal: the real input width (columns Kreal .. K - 1 of x are zero padding; dW gets zeros there).  db (optional, float32 [N]):
 * the bias gradient = column sums of dy -- only where Kreal <= 96, where it costs nothing (an all-ones operand in a padding
 * tile's place); an error otherwise (use gdl_swin_colsum). */
GDL_API int gdl_linear_bwd_ok(int dtype, size_t M, int K, int N);
GDL_API size_t gdl_linear_bwd_workspace_bytes(size_t M, int K, int N);
GDL_API int gdl_linear_bwd(int dtype, const void* dy, const void* x, const void* wT, void* dx, float* dw, float* db, void* ws,
                           size_t ws_bytes, size_t M, int K, int Kreal, int N, void* stream);
GDL_API int gdl_swin_drop_path(int dtype, const void* y, const void* res, const float* scale, void* out, size_t M, int L, int ld,
                               void* stream);
GDL_API int gdl_swin_bias_act(int dtype, void* y, const float* bias, void* u, const void* res, size_t M, int ld, int mode,
                              void* stream);
GDL_API int gdl_swin_ln_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats, size_t M,
                            int C, int ld, void* stream);
GDL_API size_t gdl_swin_partial_bytes(int ld);
GDL_API int gdl_swin_ln_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, const void* add,
                            void* dx, float* dgamma_dbeta, void* partial, size_t M, int C, int ld, void* stream);
/* the same with a third result row: dgamma_dbeta_colsum [3][ld], row 2 = column sums of dx as stored -- the bias gradient of the
 * Linear whose output gradient dx is (the residual stream's gradient feeds fc2 / proj / the patch embedding), instead of a
 * gdl_swin_colsum pass over dx.  3 * ld <= the width `partial` was sized for. */
GDL_API int gdl_swin_ln_bwd_colsum(int dtype, const void* dy, const void* x, const float* stats, const float* gamma,
                                   const void* add, void* dx, float* dgamma_dbeta_colsum, void* partial, size_t M, int C, int ld,
                                   void* stream);
GDL_API int gdl_swin_colsum(int dtype, void* g, const void* u, float* db, void* partial, size_t M, int ld, void* stream);
/* Deferred folds (round 6): gdl_swin_ln_bwd / _colsum with dgamma_dbeta == NULL and gdl_swin_colsum with db == NULL leave their
 * partial rows in `partial` -- gdl_swin_ln_bwd_rows(dtype, M, ld) rows of 2 * ld (3 * ld: _colsum) floats, gdl_swin_colsum_rows
 * (dtype, M, ld) rows of ld floats (both counts: 0 for bad arguments) -- and launch no fold; the caller gives every such call a `partial` buffer of its own and
 * folds all of them with ONE launch before the gradients are read: `descs` = device array of n_desc 32-byte records
 *   { const float* partial; float* out; int rows, width, blk0, stride; }
 * (out[j] = sum over the rows of partial[row * stride + j], j < width <= stride, in the order the per-call fold uses: bit-identical results;
 * blk0 = first block of the record, (width + 15) / 16 blocks per record, ascending; total_blocks = their sum).  The parameter
 * gradients of the reference's LayerNorms / Linear biases (swin_transformer.py:26-42,:78-157,:176-295) are only read by the
 * optimizer: 42 fold launches leave the Swin-T backward's chain. */
GDL_API int gdl_swin_ln_bwd_rows(int dtype, size_t M, int ld);
GDL_API int gdl_swin_colsum_rows(int dtype, size_t M, int ld);
GDL_API int gdl_swin_partial_reduce_batched(const void* descs, int n_desc, int total_blocks, void* stream);
GDL_API int gdl_swin_attn_fwd(int dtype, const void* qkv, const float* table, void* out, int n_img, int H, int W, int window,
                              int shift, int heads, int ld, void* stream);
GDL_API size_t gdl_swin_attn_bwd_workspace_bytes(int n_img, int H, int W, int window, int heads);
GDL_API int gdl_swin_attn_bwd(int dtype, const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable,
                              void* ws, int n_img, int H, int W, int window, int shift, int heads, int ld, void* stream);
GDL_API int gdl_swin_merge(int dtype, const void* src, void* dst, int N, int H, int W, int C, int ldx, int scatter, void* stream);
GDL_API int gdl_swin_token_mean(int dtype, const void* x, float* y, int N, int L, int C, int ld, void* stream);
GDL_API int gdl_swin_token_mean_bwd(int dtype, const float* dy, void* dx, int N, int L, int C, int ld, void* stream);
GDL_API int gdl_swin_pack_matrix(int dtype, const float* src, void* dst, void* dstT, int n, int k, int nseg, int nseg_pad,
                                 int kseg, int kseg_pad, void* stream);
/* every layout conversion of a step in one launch: `descs` = device array of n_desc 64-byte records
 *   { const float* src; void* dst; void* dstT; int n, k, nseg, nseg_pad, kseg, kseg_pad, np, kp; int dtype; int blk0; }
 * (np / kp = padded sizes, blk0 = first block of the record, 1024 elements per block, ascending; total_blocks = their sum);
 * dir 0 = gdl_swin_pack_matrix per record, dir 1 = gdl_swin_unpack_matrix per record (dstT, dtype ignored) */
GDL_API int gdl_swin_pack_batched(const void* descs, int n_desc, int total_blocks, int dir, void* stream);
GDL_API int gdl_swin_unpack_matrix(const float* src, float* dst, int n, int k, int nseg, int nseg_pad, int kseg, int kseg_pad,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel step over RCCL / xGMI (the reference's nn.DataParallel, main_dgl.py:244, as one
 * process per GPU; SURVEY 8(b) comm_init / allreduce_bucket / comm_destroy).  RCCL is bound at run time (dlopen), so the
 * library has no link-time dependency on it.  Bootstrap: rank 0 calls gdl_comm_unique_id and ships the 128 bytes to the
 * other ranks by any means (gdl/ddp.py uses the torch.distributed store); every rank then calls gdl_comm_init on ITS
 * device.  gdl_comm_allreduce_bucket sums `count` float32 gradients in place over all ranks, enqueued on `stream`
 * (collectives of one communicator execute in issue order: issue them in the same order on every rank).
 * ------------------------------------------------------------------------------------------------------------------- */
#define GDL_COMM_ID_BYTES 128
typedef struct gdl_comm gdl_comm_t;
GDL_API int gdl_comm_unique_id(void* id128);
GDL_API int gdl_comm_init(gdl_comm_t** out, int rank, int world, const void* id128);
GDL_API int gdl_comm_world(const gdl_comm_t* c);
GDL_API int gdl_comm_allreduce_bucket(gdl_comm_t* c, float* grads, size_t count, void* stream);
GDL_API int gdl_comm_destroy(gdl_comm_t* c);

#ifdef __cplusplus
}
#endif
#endif /* GDL_HIP_H */
