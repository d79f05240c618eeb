// api.cpp -- the C ABI of libgdl_hip.so (see include/gdl_hip.h) over the internal launchers.
#include "ops.h"

using namespace gdl;

#ifdef GDL_TIMING
namespace gdl { extern unsigned long long* g_timing_buf; }
#endif
extern "C" {
// tuning aid (only active in a -DGDL_TIMING build): per-block s_memtime stamps go to buf[block][8]
GDL_API int gdl_debug_timing_buffer(void* buf) {
#ifdef GDL_TIMING
    gdl::g_timing_buf = (unsigned long long*)buf;
    return GDL_OK;
#else
    (void)buf;
    return GDL_ERR_ARG;
#endif
}


const char* gdl_last_error(void) { return last_error(); }
int gdl_version(void) { return 100; }

int gdl_device_info(int* cu_count, char* name, int name_len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return check_hip(e, "hipGetDevice");
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return check_hip(e, "hipGetDeviceProperties");
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (name && name_len > 0) {
        snprintf(name, (size_t)name_len, "%s (%s)", p.name, p.gcnArchName);
    }
    return GDL_OK;
}

static bool dt_ok(int dtype) { return dtype == GDL_F32 || dtype == GDL_BF16; }

int gdl_conv_bn_tiles(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad) {
    return conv_tiles_m(dtype, ConvGeom{N, H, W, C, K, R, S, stride, pad});
}

size_t gdl_conv_table_bytes(int mode, int N, int H, int W, int R, int S, int stride, int pad) {
    return gather_table_bytes(mode, ConvGeom{N, H, W, 0, 0, R, S, stride, pad});  // (no channel count enters the size)
}
int gdl_conv_build_table(int mode, int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                         void* table, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && table && (mode == GATHER_FWD || mode == GATHER_DGRAD), "conv_build_table: bad arguments");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return build_gather_table(mode, dtype, g, (GatherEntry*)table, (hipStream_t)stream);
}
int gdl_conv_fwd(int dtype, const void* x, const void* w_krsc, void* y, float* bn_partial, const void* table, int N, int H,
                 int W, int C, int K, int R, int S, int stride, int pad, void* stream) {
    GDL_REQUIRE(x && w_krsc && y, "conv_fwd: null pointer");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_fwd(dtype, x, w_krsc, y, bn_partial, table, g, (hipStream_t)stream);
}
int gdl_bn_act_bits(int dtype, const void* y, const float* scale, const float* shift, const void* res, const float* res_scale,
                    const float* res_shift, void* out, uint8_t* relu_bits, size_t M, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && scale && shift && out && relu_bits, "bn_act_bits: bad arguments");
    return bn_act(dtype, y, scale, shift, res, res_scale, res_shift, 1, out, M, C, (hipStream_t)stream, relu_bits);
}
int gdl_conv_dgrad_relu(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, const uint8_t* relu_bits,
                        const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream) {
    GDL_REQUIRE(dy && w_crsk && dx && relu_bits, "conv_dgrad_relu: null pointer");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_dgrad(dtype, dy, w_crsk, dx, addend, table, g, (hipStream_t)stream, relu_bits);
}
int gdl_conv_fwd_bias(int dtype, const void* x, const void* w_krsc, void* y, const float* bias, const void* addend, void* gelu_out,
                      const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream) {
    GDL_REQUIRE(x && w_krsc && y, "conv_fwd_bias: null pointer");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_fwd_bias(dtype, x, w_krsc, y, bias, addend, gelu_out, table, g, (hipStream_t)stream);
}
int gdl_conv_dgrad_ds(int dtype, const void* dy, const void* w_crsk, const void* dy_ds, const void* w_ds_ck, void* dx,
                      const uint8_t* relu_bits, const void* table, int N, int H, int W, int C, int K, void* stream) {
    GDL_REQUIRE(dy && w_crsk && dy_ds && w_ds_ck && dx, "conv_dgrad_ds: null pointer");
    const ConvGeom g{N, H, W, C, K, 3, 3, 2, 1};  // conv1 of a downsample block
    return conv_dgrad_ds(dtype, dy, w_crsk, dy_ds, w_ds_ck, dx, table, g, (hipStream_t)stream, relu_bits);
}
int gdl_conv_dgrad_bn_tiles(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad) {
    return conv_dgrad_tiles_m(dtype, ConvGeom{N, H, W, C, K, R, S, stride, pad});
}
int gdl_conv_dgrad_bn(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, const uint8_t* relu_bits,
                      const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* y,
                      const float* mean, const float* rstd, float* partial, const void* y2, const float* mean2,
                      const float* rstd2, float* partial2, void* stream) {
    GDL_REQUIRE(dy && w_crsk && dx && y && mean && rstd && partial, "conv_dgrad_bn: null pointer");
    const BwdStats bw{y, mean, rstd, partial, y2, mean2, rstd2, partial2};
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_dgrad(dtype, dy, w_crsk, dx, addend, table, g, (hipStream_t)stream, relu_bits, &bw);
}
size_t gdl_conv_split_workspace_bytes(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dgrad) {
    return dt_ok(dtype) ? conv_split_ws_bytes(dtype, ConvGeom{N, H, W, C, K, R, S, stride, pad}, dgrad) : 0;
}
int gdl_conv_fwd_split(int dtype, const void* x, const void* w_krsc, void* y, float* bn_partial, const void* table, int N, int H,
                       int W, int C, int K, int R, int S, int stride, int pad, void* split_ws, size_t split_ws_bytes, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && w_krsc && y && table, "conv_fwd_split: null pointer");
    const SplitWs sk{split_ws, split_ws_bytes};
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_fwd(dtype, x, w_krsc, y, bn_partial, table, g, (hipStream_t)stream, nullptr, &sk);
}
int gdl_conv_dgrad_bn_split(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, const uint8_t* relu_bits,
                            const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, const void* y,
                            const float* mean, const float* rstd, float* partial, const void* y2, const float* mean2,
                            const float* rstd2, float* partial2, void* split_ws, size_t split_ws_bytes, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && w_crsk && dx && table, "conv_dgrad_bn_split: null pointer");
    const BwdStats bw{y, mean, rstd, partial, y2, mean2, rstd2, partial2};
    const SplitWs sk{split_ws, split_ws_bytes};
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_dgrad(dtype, dy, w_crsk, dx, addend, table, g, (hipStream_t)stream, relu_bits, y ? &bw : nullptr, &sk);
}
int gdl_conv_dgrad_gelu(int dtype, const void* dy, const void* w_crsk, void* dx, const void* u, void* acc, double scale,
                        const void* table, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && w_crsk && dx && u && acc && table && scale > 0.0, "conv_dgrad_gelu: bad arguments");
    const BnAcc a{(long long*)acc, scale, 0.0};
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_dgrad_gelu(dtype, dy, w_crsk, dx, u, &a, table, g, (hipStream_t)stream);
}
int gdl_acc_to_float(const void* acc, int n, double inv_scale, float* out, void* stream) {
    GDL_REQUIRE(acc && out && n > 0, "acc_to_float: bad arguments");
    return acc_to_float((const long long*)acc, n, inv_scale, out, (hipStream_t)stream);
}
int gdl_conv_dgrad(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, const void* table, int N,
                   int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream) {
    GDL_REQUIRE(dy && w_crsk && dx, "conv_dgrad: null pointer");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_dgrad(dtype, dy, w_crsk, dx, addend, table, g, (hipStream_t)stream);
}
size_t gdl_conv_wgrad_workspace_bytes(int dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad) {
    (void)dtype;
    return conv_wgrad_ws_bytes(ConvGeom{N, H, W, C, K, R, S, stride, pad});
}
int gdl_conv_wgrad(int dtype, const void* dy, const void* x, float* dw, const void* table, int N, int H, int W, int C,
                   int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(dy && x && dw, "conv_wgrad: null pointer");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    return conv_wgrad(dtype, dy, x, dw, table, g, C, ws, ws_bytes, (hipStream_t)stream);
}
int gdl_pack_weight(int dtype, const float* w, void* w_krsc, void* w_crsk, int K, int C, int R, int S, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && w, "pack_weight: bad arguments");
    return pack_weight(dtype, w, w_krsc, w_crsk, K, C, R, S, (hipStream_t)stream);
}
// direct stem
size_t gdl_stem_pad_bytes(int dtype, int n_img, int H, int W) { return dt_ok(dtype) ? stem_pad_bytes(dtype, n_img, H, W) : 0; }
size_t gdl_stem_weight_bytes(int dtype) {
    return dt_ok(dtype) ? (size_t)64 * stem_taps(dtype) * stem_ic(dtype) * (dtype == GDL_BF16 ? 2 : 4) : 0;
}
size_t gdl_stem_table_bytes(int n_img, int H, int W) {
    return (size_t)n_img * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * sizeof(GatherEntry);
}
int gdl_stem_pad(int dtype, const float* x, void* xp, int B, int Cin, int T, int H, int W, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && xp, "stem_pad: bad arguments");
    return stem_pad(dtype, x, xp, B, Cin, T, H, W, (hipStream_t)stream);
}
int gdl_pack_stem_rows(int dtype, const float* w, void* wp, int Cin, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && w && wp && Cin >= 1 && Cin <= 4, "pack_stem_rows: bad arguments");
    return pack_stem_rows(dtype, w, wp, Cin, (hipStream_t)stream);
}
int gdl_stem_build_table(int dtype, int n_img, int H, int W, void* table, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && table, "stem_build_table: bad arguments");
    return build_stem_table(dtype, n_img, H, W, stem_taps(dtype), (GatherEntry*)table, (hipStream_t)stream);
}
int gdl_stem_conv_bn_tiles(int dtype, int n_img, int H, int W) { return conv_stem_tiles_m(dtype, n_img, H, W); }
int gdl_stem_conv_fwd(int dtype, const void* xp, const void* wp, void* y, float* bn_partial, const void* table, int n_img,
                      int H, int W, int Cin, void* stream) {
    GDL_REQUIRE(dt_ok(dtype), "stem_conv_fwd: bad dtype");
    return conv_stem_fwd(dtype, xp, wp, y, bn_partial, table, n_img, H, W, Cin, (hipStream_t)stream);
}
size_t gdl_stem_conv_wgrad_workspace_bytes(int n_img, int H, int W) { return conv_stem_wgrad_ws_bytes(n_img, H, W); }
int gdl_stem_bwd_fused_ok(int dtype, int W) { return stem_bwd_fused_ok(dtype, W) ? 1 : 0; }
int gdl_stem_bwd_fused(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* scale, const float* shift,
                       const float* save_mean, const float* save_rstd, const float* gamma, const float* coef, const void* xp,
                       float* dw, int n_img, int H, int W, int Cin, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(stem_bwd_fused_ok(dtype, W), "stem_bwd_fused: bf16 with output rows of at least 64 pixels only (ask gdl_stem_bwd_fused_ok)");
    return stem_bwd_fused(dout, idx, y, scale, shift, save_mean, save_rstd, gamma, coef, xp, dw, n_img, H, W, Cin, ws, ws_bytes,
                          (hipStream_t)stream);
}
int gdl_stem_conv_wgrad(int dtype, const void* dy, const void* xp, float* dw, const void* table, int n_img, int H, int W,
                        int Cin, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && Cin >= 1 && Cin <= 4, "stem_conv_wgrad: bad arguments");
    return conv_stem_wgrad(dtype, dy, xp, dw, table, n_img, H, W, Cin, ws, ws_bytes, (hipStream_t)stream);
}
int gdl_nhwc_to_nchw_f32(int dtype, const void* x, float* y, int N, int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && y, "nhwc_to_nchw: bad arguments");
    return nhwc_to_nchw_f32(dtype, x, y, N, H, W, C, (hipStream_t)stream);
}
int gdl_nchw_f32_to_nhwc(int dtype, const float* x, void* y, int N, int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && y, "nchw_to_nhwc: bad arguments");
    return nchw_f32_to_nhwc(dtype, x, y, N, H, W, C, (hipStream_t)stream);
}

int gdl_bn_stats_tiles(int M) { return bn_stats_tiles(M); }
int gdl_bn_stats(int dtype, const void* y, float* partial, int M, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && partial, "bn_stats: bad arguments");
    return bn_stats(dtype, y, partial, M, C, (hipStream_t)stream);
}
int gdl_bn_finalize_train(const float* partial, int tiles, int C, double count, const float* gamma, const float* beta,
                          float eps, float momentum, float* running_mean, float* running_var, int64_t* nbt,
                          float* save_mean, float* save_rstd, float* scale, float* shift, void* stream) {
    GDL_REQUIRE(partial && gamma && beta && save_mean && save_rstd && scale && shift, "bn_finalize_train: null pointer");
    return bn_finalize_train(partial, tiles, C, count, gamma, beta, eps, momentum, running_mean, running_var, nbt,
                             save_mean, save_rstd, scale, shift, (hipStream_t)stream);
}
int gdl_bn_finalize_eval(int C, const float* gamma, const float* beta, float eps, const float* running_mean,
                         const float* running_var, float* scale, float* shift, void* stream) {
    GDL_REQUIRE(gamma && beta && running_mean && running_var && scale && shift, "bn_finalize_eval: null pointer");
    return bn_finalize_eval(C, gamma, beta, eps, running_mean, running_var, scale, shift, (hipStream_t)stream);
}
int gdl_bn_act(int dtype, const void* y, const float* scale, const float* shift, const void* res, const float* res_scale,
               const float* res_shift, int relu, void* out, size_t M, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && scale && shift && out, "bn_act: bad arguments");
    return bn_act(dtype, y, scale, shift, res, res_scale, res_shift, relu, out, M, C, (hipStream_t)stream);
}
int gdl_bn_bwd_blocks(size_t M, int C) { return bn_bwd_blocks(M, C); }
int gdl_bn_bwd_reduce(int dtype, const void* g, const void* y, const float* scale, const float* shift,
                      const float* save_mean, const float* save_rstd, int relu_mask, float* partial, size_t M, int C,
                      void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && g && y && save_mean && save_rstd && partial, "bn_bwd_reduce: bad arguments");
    return bn_bwd_reduce(dtype, g, y, scale, shift, save_mean, save_rstd, relu_mask, partial, M, C, (hipStream_t)stream);
}
int gdl_bn_bwd_finalize(const float* partial, int blocks, int C, double count, float* dgamma, float* dbeta, float* coef,
                        void* stream) {
    GDL_REQUIRE(partial && dgamma && dbeta && coef, "bn_bwd_finalize: null pointer");
    return bn_bwd_finalize(partial, blocks, C, count, dgamma, dbeta, coef, (hipStream_t)stream);
}
int gdl_bn_bwd_apply(int dtype, const void* g, const void* y, const float* scale, const float* shift,
                     const float* save_mean, const float* save_rstd, const float* gamma, const float* coef, int relu_mask,
                     void* dy, size_t M, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && g && y && save_mean && save_rstd && gamma && coef && dy, "bn_bwd_apply: bad arguments");
    return bn_bwd_apply(dtype, g, y, scale, shift, save_mean, save_rstd, gamma, coef, relu_mask, dy, M, C,
                        (hipStream_t)stream);
}
int gdl_relu_bwd(int dtype, const void* dy, const void* out, void* dx, size_t n, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && out && dx, "relu_bwd: bad arguments");
    return relu_bwd(dtype, dy, out, dx, n, (hipStream_t)stream);
}

int gdl_bn_relu_maxpool_fwd(int dtype, const void* y, const float* scale, const float* shift, void* out, uint8_t* idx,
                            void* ymax, int N, int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && scale && shift && out && idx, "bn_relu_maxpool_fwd: bad arguments");
    return bn_relu_maxpool_fwd(dtype, y, scale, shift, out, idx, ymax, N, H, W, C, (hipStream_t)stream);
}
// ---- the fused forms the encoder engine launches, one entry point per kernel so that each can be tested alone
// (tests/test_bnacc_gpu.py).  Accumulator buffers follow the engine's arena convention: int64 [C][2] + one flag word.
static BnAcc acc_producer_of(int64_t* acc, int C, size_t rows) {
    BnAcc a{(long long*)acc, 0.0, 0.0, (long long*)acc + 2 * (size_t)C};
    bn_acc_scales(rows, &a.s1, &a.s2);
    return a;
}
static BnAccFin acc_consumer_of(const int64_t* acc, int C, size_t rows, const float* gamma, const float* beta, float* rm, float* rv,
                                int64_t* nbt, float* save_mean, float* save_rstd, float* scale, float* shift, float eps,
                                float momentum) {
    double s1, s2;
    bn_acc_scales(rows, &s1, &s2);
    return BnAccFin{(const long long*)acc, 1.0 / s1, 1.0 / s2, (double)rows, gamma, beta, rm, rv, nbt, save_mean, save_rstd, scale,
                    shift, eps, momentum, acc ? (const long long*)acc + 2 * (size_t)C : nullptr};
}
int gdl_bn_acc_scales(size_t rows, double* s1, double* s2) {
    GDL_REQUIRE(s1 && s2 && rows >= 1, "bn_acc_scales: bad arguments");
    bn_acc_scales(rows, s1, s2);
    return GDL_OK;
}
int gdl_conv_fwd_acc(int dtype, const void* x, const void* w_krsc, void* y, int64_t* acc, const void* table, int N, int H, int W,
                     int C, int K, int R, int S, int stride, int pad, void* split_ws, size_t split_ws_bytes, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && w_krsc && y && acc && stride >= 1, "conv_fwd_acc: bad arguments");
    const ConvGeom g{N, H, W, C, K, R, S, stride, pad};
    const size_t rows = (size_t)N * ((H + 2 * pad - R) / stride + 1) * ((W + 2 * pad - S) / stride + 1);
    const BnAcc a = acc_producer_of(acc, K, rows);
    const SplitWs sk{split_ws, split_ws_bytes};
    return conv_fwd(dtype, x, w_krsc, y, nullptr, table, g, (hipStream_t)stream, &a, split_ws ? &sk : nullptr);
}
int gdl_stem_conv_fwd_acc(int dtype, const void* xp, const void* wp, void* y, int64_t* acc, const void* table, int n_img, int H,
                          int W, int Cin, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && acc, "stem_conv_fwd_acc: bad arguments");
    const BnAcc a = acc_producer_of(acc, 64, (size_t)n_img * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1));
    return conv_stem_fwd(dtype, xp, wp, y, nullptr, table, n_img, H, W, Cin, (hipStream_t)stream, &a);
}
int gdl_stem_pad_zero(int dtype, const float* x, void* xp, int B, int Cin, int T, int H, int W, void* zero, size_t zero_bytes,
                      void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && xp && (zero || zero_bytes == 0), "stem_pad_zero: bad arguments");
    return stem_pad(dtype, x, xp, B, Cin, T, H, W, (hipStream_t)stream, zero, zero_bytes);
}
int gdl_bn_act_acc(int dtype, const void* y, const int64_t* acc, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, int64_t* nbt, float* save_mean, float* save_rstd, float* scale, float* shift,
                   const void* res, const int64_t* res_acc, const float* res_gamma, const float* res_beta,
                   float* res_running_mean, float* res_running_var, int64_t* res_nbt, float* res_save_mean, float* res_save_rstd,
                   float* res_scale, float* res_shift, size_t rows, float eps, float momentum, int relu, void* out,
                   uint8_t* relu_bits, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && acc && gamma && beta && save_mean && save_rstd && scale && shift && out && rows >= 1,
                "bn_act_acc: bad arguments");
    GDL_REQUIRE((res_scale == nullptr) == (res_shift == nullptr) && (res || !res_scale), "bn_act_acc: residual constants without a residual");
    GDL_REQUIRE(!res_acc || (res_scale && res_gamma && res_beta && res_save_mean && res_save_rstd),
                "bn_act_acc: residual accumulators need gamma / beta / saved statistics / scale / shift");
    const BnAccFin fa = acc_consumer_of(acc, C, rows, gamma, beta, running_mean, running_var, nbt, save_mean, save_rstd, scale, shift,
                                        eps, momentum);
    const BnAccFin fr = acc_consumer_of(res_acc, C, rows, res_gamma, res_beta, res_running_mean, res_running_var, res_nbt,
                                        res_save_mean, res_save_rstd, res_scale, res_shift, eps, momentum);
    return bn_act(dtype, y, scale, shift, res, res_scale, res_shift, relu, out, rows, C, (hipStream_t)stream, relu_bits, &fa,
                  res_scale ? &fr : nullptr);
}
int gdl_bn_relu_maxpool_fwd_acc(int dtype, const void* y, const int64_t* acc, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* nbt, float* save_mean, float* save_rstd,
                                float* scale, float* shift, float eps, float momentum, void* out, uint8_t* idx, void* ymax, int N,
                                int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && acc && gamma && beta && save_mean && save_rstd && scale && shift && out && idx,
                "bn_relu_maxpool_fwd_acc: bad arguments");
    const BnAccFin fa = acc_consumer_of(acc, C, (size_t)N * H * W, gamma, beta, running_mean, running_var, nbt, save_mean, save_rstd,
                                        scale, shift, eps, momentum);
    return bn_relu_maxpool_fwd(dtype, y, scale, shift, out, idx, ymax, N, H, W, C, (hipStream_t)stream, &fa);
}
int gdl_block_bwd_reduce(int dtype, const void* dz, const void* z, const void* y2, const void* yd, const float* mean2,
                         const float* rstd2, const float* meand, const float* rstdd, void* do2, float* partial2, float* partiald,
                         size_t M, int C, int premasked, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dz && y2 && mean2 && rstd2 && partial2, "block_bwd_reduce: bad arguments");
    GDL_REQUIRE(!yd || (meand && rstdd && partiald), "block_bwd_reduce: downsample branch without its statistics / partial rows");
    return block_bwd_reduce(dtype, dz, z, y2, yd, mean2, rstd2, meand, rstdd, do2, partial2, partiald, M, C, (hipStream_t)stream,
                            premasked != 0);
}
int gdl_bn_bwd_apply2(int dtype, const void* g, const void* yA, const float* meanA, const float* rstdA, const float* gammaA,
                      const float* coefA, void* dyA, const void* yB, const float* meanB, const float* rstdB, const float* gammaB,
                      const float* coefB, void* dyB, size_t M, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && g && yA && meanA && rstdA && gammaA && coefA && dyA && yB && meanB && rstdB && gammaB && coefB && dyB,
                "bn_bwd_apply2: bad arguments");
    GDL_REQUIRE(C > 0 && C % (dtype == GDL_BF16 ? 8 : 4) == 0, "bn_bwd_apply2: C=%d unsupported", C);
    return bn_bwd_apply2(dtype, g, yA, meanA, rstdA, gammaA, coefA, dyA, yB, meanB, rstdB, gammaB, coefB, dyB, M, C,
                         (hipStream_t)stream);
}
int gdl_bn_finalize_train_pair(const float* partialA, int tilesA, double countA, const float* gammaA, const float* betaA,
                               float* running_meanA, float* running_varA, int64_t* nbtA, float* save_meanA, float* save_rstdA,
                               float* scaleA, float* shiftA, const float* partialB, int tilesB, double countB, const float* gammaB,
                               const float* betaB, float* running_meanB, float* running_varB, int64_t* nbtB, float* save_meanB,
                               float* save_rstdB, float* scaleB, float* shiftB, int C, float eps, float momentum, void* stream) {
    GDL_REQUIRE(partialA && gammaA && betaA && save_meanA && save_rstdA && scaleA && shiftA && partialB && gammaB && betaB &&
                    save_meanB && save_rstdB && scaleB && shiftB,
                "bn_finalize_train_pair: null pointer");
    const BnFinTrain a{partialA, tilesA, C, countA, gammaA, betaA, running_meanA, running_varA, nbtA, save_meanA, save_rstdA, scaleA, shiftA};
    const BnFinTrain b{partialB, tilesB, C, countB, gammaB, betaB, running_meanB, running_varB, nbtB, save_meanB, save_rstdB, scaleB, shiftB};
    return bn_finalize_train_pair(a, b, eps, momentum, (hipStream_t)stream);
}
int gdl_bn_bwd_finalize_pair(const float* partialA, int blocksA, double countA, float* dgammaA, float* dbetaA, float* coefA,
                             const float* partialB, int blocksB, double countB, float* dgammaB, float* dbetaB, float* coefB, int C,
                             void* stream) {
    GDL_REQUIRE(partialA && dgammaA && dbetaA && coefA && partialB && dgammaB && dbetaB && coefB, "bn_bwd_finalize_pair: null pointer");
    const BnFinBwd a{partialA, blocksA, C, countA, dgammaA, dbetaA, coefA}, b{partialB, blocksB, C, countB, dgammaB, dbetaB, coefB};
    return bn_bwd_finalize_pair(a, b, (hipStream_t)stream);
}
int gdl_maxpool_bn_bwd_apply(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* scale,
                             const float* shift, const float* save_mean, const float* save_rstd, const float* gamma,
                             const float* coef, void* dy, int N, int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dout && idx && y && scale && shift && save_mean && save_rstd && gamma && coef && dy,
                "maxpool_bn_bwd_apply: bad arguments");
    return maxpool_bn_bwd_apply(dtype, dout, idx, y, scale, shift, save_mean, save_rstd, gamma, coef, dy, N, H, W, C,
                                (hipStream_t)stream);
}
int gdl_maxpool_bwd(int dtype, const void* dout, const uint8_t* idx, void* dx, int N, int H, int W, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dout && idx && dx, "maxpool_bwd: bad arguments");
    return maxpool_bwd(dtype, dout, idx, dx, N, H, W, C, (hipStream_t)stream);
}
int gdl_avgpool_fwd(int dtype, const void* x, float* feat, int B, int T, int HW, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && feat, "avgpool_fwd: bad arguments");
    return avgpool_fwd(dtype, x, feat, B, T, HW, C, (hipStream_t)stream);
}
int gdl_avgpool_bwd(int dtype, const float* dfeat, void* dx, int B, int T, int HW, int C, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dfeat && dx, "avgpool_bwd: bad arguments");
    return avgpool_bwd(dtype, dfeat, dx, B, T, HW, C, (hipStream_t)stream);
}

int gdl_head_uni_dfeat(const float* f, const float* Wp, int ldw, const float* bp, const int64_t* labels, float scale, float* df,
                       int B, int n_classes, void* stream) {
    GDL_REQUIRE(f && Wp && bp && labels && df && B > 0 && n_classes > 0 && ldw >= 512, "head_uni_dfeat: bad arguments");
    return head_uni_dfeat(f, Wp, ldw, bp, labels, scale, df, B, n_classes, 512, (hipStream_t)stream);
}
int gdl_head_uni_dfeat_w(const float* f, const float* Wp, int ldw, const float* bp, const int64_t* labels, float scale, float* df,
                         int B, int n_classes, int width, void* stream) {
    GDL_REQUIRE(f && Wp && bp && labels && df && B > 0 && n_classes > 0 && ldw >= width, "head_uni_dfeat_w: bad arguments");
    return head_uni_dfeat(f, Wp, ldw, bp, labels, scale, df, B, n_classes, width, (hipStream_t)stream);
}
size_t gdl_head_uni_scores_workspace_bytes(void) { return 16; }
int gdl_head_uni_scores(const float* fa, const float* fv, const float* Wa, const float* Wv, int ldw, const float* ba,
                        const float* bv, float bias_scale, const int64_t* labels, float* prob, float* scores, int B,
                        int n_classes, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(fa && fv && Wa && Wv && ba && bv && labels && prob && scores && ws && B > 0 && n_classes > 0 && ldw >= 512,
                "head_uni_scores: bad arguments");
    GDL_REQUIRE(ws_bytes >= gdl_head_uni_scores_workspace_bytes() && ((uintptr_t)ws & 3) == 0,
                "head_uni_scores: workspace of %zu bytes, 4-byte aligned", gdl_head_uni_scores_workspace_bytes());
    return head_uni_scores(fa, fv, Wa, Wv, ldw, ba, bv, bias_scale, labels, prob, scores, B, n_classes, ws, (hipStream_t)stream);
}
int gdl_head_cls_fwd(const float* f, const float* W, const float* b, float* out, int B, int n_classes, int width, void* stream) {
    GDL_REQUIRE(f && W && b && out && B > 0 && n_classes > 0, "head_cls_fwd: bad arguments");
    GDL_REQUIRE(width == 512, "head_cls_fwd: feature width %d (the classifier is built for 512)", width);
    return head_cls_fwd(f, W, b, out, B, n_classes, (hipStream_t)stream);
}
int gdl_head_cls_bwd(const float* f, const float* W, const float* g_out, float* df, float* dW, float* db, int B, int n_classes,
                     int width, void* stream) {
    GDL_REQUIRE(f && W && g_out && B > 0 && n_classes > 0, "head_cls_bwd: bad arguments");
    GDL_REQUIRE(width == 512, "head_cls_bwd: feature width %d (the classifier is built for 512)", width);
    return head_cls_bwd(f, W, g_out, df, dW, db, B, n_classes, (hipStream_t)stream);
}
int gdl_head_cls_ce(const float* f, const float* W, const float* b, const int64_t* labels, float scale, float* out, float* loss,
                    float* dlogits, float* df, int B, int n_classes, int width, void* stream) {
    GDL_REQUIRE(f && W && b && labels && out && loss && dlogits && df && B > 0 && n_classes > 0, "head_cls_ce: bad arguments");
    GDL_REQUIRE(width == 512, "head_cls_ce: feature width %d (the classifier is built for 512)", width);
    return head_cls_ce(f, W, b, labels, scale, out, loss, dlogits, df, B, n_classes, (hipStream_t)stream);
}
size_t gdl_linprobe_workspace_bytes(int B, int n_classes) { return linprobe_ws_bytes(B, n_classes); }
int gdl_linprobe_epoch(const float* bank, const int64_t* labels, int64_t N, const int32_t* order, int steps, int B, float* W,
                       float* b, float* mW, float* mb, int n_classes, float lr, float momentum, float weight_decay, float max_norm,
                       double* loss_acc, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(n_classes >= 1 && n_classes <= 512, "linprobe_epoch: n_classes must be in [1, 512] (Linear(512, n)), got %d", n_classes);
    GDL_REQUIRE(B >= 1 && steps >= 0 && N >= 1, "linprobe_epoch: B = %d (>= 1), steps = %d (>= 0), N = %lld (>= 1)", B, steps, (long long)N);
    GDL_REQUIRE(bank && labels && W && b && mW && mb && loss_acc && ws && (order || steps == 0), "linprobe_epoch: null argument");
    GDL_REQUIRE((((uintptr_t)W | (uintptr_t)mW | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)loss_acc & 7) == 0,
                "linprobe_epoch: W, mW and ws must be 16-byte aligned, loss_acc 8-byte aligned");
    if (ws_bytes < linprobe_ws_bytes(B, n_classes)) {
        set_error("linprobe_epoch: workspace %zu < %zu", ws_bytes, linprobe_ws_bytes(B, n_classes));
        return GDL_ERR_WORKSPACE;
    }
    return linprobe_epoch(bank, labels, N, order, steps, B, W, b, mW, mb, n_classes, lr, momentum, weight_decay, max_norm, loss_acc,
                          ws, (hipStream_t)stream);
}
int gdl_proto_ce(const float* f, const float* P, const int64_t* labels, float* u, float* terms, float* sim, int B, int n_classes,
                 int width, void* stream) {
    GDL_REQUIRE(width == 512, "proto_ce: feature width %d (the prototypes are built for 512)", width);
    GDL_REQUIRE(n_classes >= 1 && n_classes <= 512, "proto_ce: n_classes must be in [1, 512], got %d", n_classes);
    GDL_REQUIRE(B >= 1, "proto_ce: B must be at least 1, got %d", B);
    GDL_REQUIRE(f && P && labels && u && terms, "proto_ce: null argument (only sim may be NULL)");
    return proto_ce(f, P, labels, u, terms, sim, B, n_classes, (hipStream_t)stream);
}
int gdl_proto_apply(const float* terms_a, const float* terms_v, const float* u_a, const float* u_v, float* dfa, float* dfv,
                    float alpha, float* stats, int B, int width, void* stream) {
    GDL_REQUIRE(width == 512, "proto_apply: feature width %d (the prototypes are built for 512)", width);
    GDL_REQUIRE(B >= 1 && B <= (1 << 22), "proto_apply: B must be in [1, 2^22], got %d", B);
    GDL_REQUIRE(terms_a && terms_v && u_a && u_v && dfa && dfv && stats, "proto_apply: null argument");
    GDL_REQUIRE((((uintptr_t)u_a | (uintptr_t)u_v | (uintptr_t)dfa | (uintptr_t)dfv) & 15) == 0,
                "proto_apply: u_a, u_v, dfa and dfv must be 16-byte aligned");
    return proto_apply(terms_a, terms_v, u_a, u_v, dfa, dfv, alpha, stats, B, (hipStream_t)stream);
}
int gdl_proto_update(const float* bank, const int64_t* labels, int64_t N, float* P, int n_classes, int width, double momentum,
                     int first, int64_t* count, int64_t* info, void* stream) {
    GDL_REQUIRE(width == 512, "proto_update: feature width %d (the prototypes are built for 512)", width);
    GDL_REQUIRE(n_classes >= 1 && n_classes <= 512, "proto_update: n_classes must be in [1, 512], got %d", n_classes);
    GDL_REQUIRE(N >= 1, "proto_update: N must be at least 1, got %lld", (long long)N);
    GDL_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "proto_update: momentum must be in [0, 1], got %g", momentum);
    GDL_REQUIRE(bank && labels && P && count && info, "proto_update: null argument");
    return proto_update(bank, labels, N, P, n_classes, momentum, first != 0, count, info, (hipStream_t)stream);
}
int gdl_mla_feature_mean(const float* h, int B, float* r, void* stream) {
    GDL_REQUIRE(B >= 1, "mla_feature_mean: B must be at least 1, got %d", B);
    GDL_REQUIRE(h && r, "mla_feature_mean: null argument");
    return mla_feature_mean(h, B, r, (hipStream_t)stream);
}
size_t gdl_mla_projector_workspace_bytes(void) { return mla_projector_ws_bytes(); }
int gdl_mla_projector_update(float* P, const float* r, float alpha, int normalize, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(P && r && ws, "mla_projector_update: null argument");
    GDL_REQUIRE(alpha > 0.f && alpha <= 3.0e38f, "mla_projector_update: alpha must be a finite positive number, got %g", (double)alpha);
    GDL_REQUIRE(ws_bytes >= mla_projector_ws_bytes(), "mla_projector_update: workspace %zu < %zu", ws_bytes, mla_projector_ws_bytes());
    GDL_REQUIRE(((uintptr_t)ws & 3) == 0, "mla_projector_update: the workspace must be 4-byte aligned");
    return mla_projector_update(P, r, alpha, normalize != 0, ws, (hipStream_t)stream);
}
int gdl_mla_project(float* dW, const float* P, int n_classes, void* stream) {
    GDL_REQUIRE(n_classes >= 1 && n_classes <= 512, "mla_project: n_classes must be in [1, 512], got %d", n_classes);
    GDL_REQUIRE(dW && P, "mla_project: null argument");
    return mla_project(dW, P, n_classes, (hipStream_t)stream);
}
int gdl_mla_fuse(const float* out_a, const float* out_v, int B, int n_classes, int dynamic, float* out, float* lam, void* stream) {
    GDL_REQUIRE(n_classes >= 1 && n_classes <= 512, "mla_fuse: n_classes must be in [1, 512], got %d", n_classes);
    GDL_REQUIRE(B >= 1, "mla_fuse: B must be at least 1, got %d", B);
    GDL_REQUIRE(out_a && out_v && out, "mla_fuse: null argument (only lam may be NULL)");
    return mla_fuse(out_a, out_v, B, n_classes, dynamic != 0, out, lam, (hipStream_t)stream);
}
size_t gdl_pareto_workspace_bytes(int64_t n) { return pareto_ws_bytes(n); }
int gdl_pareto_integrate(float* g_m, const float* g_u, int64_t n, float scale, float* info, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(n >= 1 && n <= ((int64_t)1 << 36), "pareto_integrate: n must be in [1, 2^36], got %lld", (long long)n);
    GDL_REQUIRE(g_m && g_u && info && ws, "pareto_integrate: null argument");
    GDL_REQUIRE((((uintptr_t)g_m | (uintptr_t)g_u | (uintptr_t)info) & 3) == 0, "pareto_integrate: g_m, g_u and info must be 4-byte aligned");
    GDL_REQUIRE(((uintptr_t)ws & 15) == 0, "pareto_integrate: the workspace must be 16-byte aligned");
    GDL_REQUIRE(ws_bytes >= pareto_ws_bytes(n), "pareto_integrate: workspace %zu < %zu", ws_bytes, pareto_ws_bytes(n));
    return pareto_integrate(g_m, g_u, n, scale, info, ws, (hipStream_t)stream);
}
size_t gdl_feature_diversity_workspace_bytes(int n_img) { return feature_diversity_ws_bytes(n_img); }
int gdl_feature_diversity(const void* map, int dtype, int layout, int n_img, int P, int C, float* per_image, float* mean_out,
                          float* accum, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(map && mean_out && ws, "feature_diversity: null map, mean_out or workspace");
    GDL_REQUIRE(dt_ok(dtype) && (layout == GDL_LAYOUT_NHWC || layout == GDL_LAYOUT_NCHW), "feature_diversity: dtype %d, layout %d",
                dtype, layout);
    GDL_REQUIRE(C == 512, "feature_diversity: built for C = 512 channels (the ResNet18 encoders' final map), got %d", C);
    GDL_REQUIRE(P >= 1 && P <= 256, "feature_diversity: P = h w must be in [1, 256], got %d", P);
    GDL_REQUIRE(n_img >= 1, "feature_diversity: n_img must be at least 1, got %d", n_img);
    GDL_REQUIRE(!(layout == GDL_LAYOUT_NCHW && dtype != GDL_F32), "feature_diversity: the NCHW layout is float32 only (bf16 maps are NHWC)");
    GDL_REQUIRE(((uintptr_t)map & (layout == GDL_LAYOUT_NHWC ? 15 : 3)) == 0, "feature_diversity: map must be %d-byte aligned",
                layout == GDL_LAYOUT_NHWC ? 16 : 4);
    GDL_REQUIRE(ws_bytes >= feature_diversity_ws_bytes(n_img) && ((uintptr_t)ws & 255) == 0,
                "feature_diversity: workspace of %zu bytes, 256-byte aligned", feature_diversity_ws_bytes(n_img));
    return feature_diversity(map, dtype, layout, n_img, P, per_image, mean_out, accum, ws, (hipStream_t)stream);
}
size_t gdl_journal_bytes(int64_t capacity) { return journal_bytes(capacity); }
int gdl_journal_append(void* journal, int64_t capacity, const float* losses, int n_losses, const float* stats, const float* out_a,
                       const float* out_v, int64_t n_logits, const float* div_a, const float* div_v, const float* ogm,
                       void* stream) {
    GDL_REQUIRE(journal, "journal_append: null journal");
    GDL_REQUIRE(capacity >= 1, "journal_append: capacity must be at least 1 row, got %lld", (long long)capacity);
    GDL_REQUIRE(n_losses == 1 || n_losses == 3, "journal_append: n_losses must be 3, or 1 (the one loss in all three columns), got %d",
                n_losses);
    GDL_REQUIRE(losses && stats, "journal_append: null losses or stats");
    GDL_REQUIRE(n_logits >= 0, "journal_append: n_logits must not be negative, got %lld", (long long)n_logits);
    GDL_REQUIRE(n_logits > 0 || (!out_a && !out_v), "journal_append: out_a / out_v given with n_logits = 0 (the mean of no values)");
    GDL_REQUIRE(((uintptr_t)journal & 15) == 0, "journal_append: the journal must be 16-byte aligned");
    return journal_append(journal, capacity, losses, n_losses, stats, out_a, out_v, n_logits, div_a, div_v, ogm,
                          (hipStream_t)stream);
}
size_t gdl_eval_bank_bytes(int n_classes, int64_t capacity, int sets) { return eval_bank_bytes(n_classes, capacity, sets); }
size_t gdl_eval_bank_reset_bytes(int n_classes, int sets) { return eval_bank_reset_bytes(n_classes, sets); }
// the checks the two score-bank calls share: 0 when the bank can be used as described
static int eval_bank_check(const char* who, const void* bank, size_t bank_bytes, int n, int64_t capacity, int sets) {
    GDL_REQUIRE(bank, "%s: null bank", who);
    GDL_REQUIRE(n >= 1 && n <= 512, "%s: n_classes must be in [1, 512], got %d", who, n);
    GDL_REQUIRE(sets == 1 || sets == 3, "%s: sets must be 1 (fused alone) or 3 (fused, audio, visual), got %d", who, sets);
    GDL_REQUIRE(capacity >= 1 && capacity < ((int64_t)1 << 31), "%s: capacity must be in [1, 2^31), got %lld", who,
                (long long)capacity);
    GDL_REQUIRE(bank_bytes >= eval_bank_bytes(n, capacity, sets), "%s: a bank of %zu bytes, gdl_eval_bank_bytes asks for %zu", who,
                bank_bytes, eval_bank_bytes(n, capacity, sets));
    GDL_REQUIRE(((uintptr_t)bank & 15) == 0, "%s: the bank must be 16-byte aligned", who);
    return GDL_OK;
}
int gdl_eval_bank_append(void* bank, size_t bank_bytes, int n_classes, int64_t capacity, int sets, const float* out,
                         const float* out_a, const float* out_v, const int64_t* labels, int B, int64_t offset, void* stream) {
    if (int rc = eval_bank_check("eval_bank_append", bank, bank_bytes, n_classes, capacity, sets)) return rc;
    GDL_REQUIRE(out && labels, "eval_bank_append: null out or labels");
    GDL_REQUIRE(sets == 3 || (!out_a && !out_v), "eval_bank_append: a unimodal logit set given to a bank of sets = 1");
    GDL_REQUIRE(sets == 1 || (out_a && out_v), "eval_bank_append: a bank of sets = 3 needs out_a and out_v");
    GDL_REQUIRE(B >= 1, "eval_bank_append: B must be at least 1, got %d", B);
    GDL_REQUIRE(offset >= 0 && offset + B <= capacity, "eval_bank_append: rows %lld .. %lld do not fit a capacity of %lld",
                (long long)offset, (long long)offset + B - 1, (long long)capacity);
    return eval_bank_append(bank, n_classes, capacity, sets, out, out_a, out_v, labels, B, offset, (hipStream_t)stream);
}
int gdl_eval_bank_ap(void* bank, size_t bank_bytes, int n_classes, int64_t capacity, int sets, int64_t N, void* stream) {
    if (int rc = eval_bank_check("eval_bank_ap", bank, bank_bytes, n_classes, capacity, sets)) return rc;
    GDL_REQUIRE(N >= 0 && N <= capacity, "eval_bank_ap: N = %lld samples in a bank of capacity %lld", (long long)N,
                (long long)capacity);
    return eval_bank_ap(bank, n_classes, capacity, sets, N, (hipStream_t)stream);
}
size_t gdl_head_mtl_ce_workspace_bytes(int B) { return head_mtl_ce_ws_bytes(B); }
int gdl_head_mtl_ce(const float* fa, const float* fv, const float* Wa, const float* Wv, int ldw, const float* ba, const float* bv,
                    int sum_bias, const int64_t* labels, float scale_u, int fused_reaches, float* out, float* out_a, float* out_v,
                    float* losses, float* g_f, float* g_a, float* g_v, float* dfa, float* dfv, int B, int n_classes, void* ws,
                    size_t ws_bytes, void* stream) {
    GDL_REQUIRE(fa && fv && Wa && Wv && ba && bv && labels && out && out_a && out_v && losses && g_f && g_a && g_v && dfa && dfv &&
                    ws && B > 0 && n_classes > 0 && ldw >= 512,
                "head_mtl_ce: bad arguments");
    GDL_REQUIRE(ws_bytes >= head_mtl_ce_ws_bytes(B) && ((uintptr_t)ws & 3) == 0, "head_mtl_ce: workspace of %zu bytes, 4-byte aligned",
                head_mtl_ce_ws_bytes(B));
    return head_mtl_ce(fa, fv, Wa, Wv, ldw, ba, bv, sum_bias != 0, labels, scale_u, fused_reaches != 0, out, out_a, out_v, losses, g_f,
                       g_a, g_v, dfa, dfv, B, n_classes, ws, (hipStream_t)stream);
}
int gdl_head_concat_fwd(const float* x, const float* y, const float* W, const float* b, float* out, float* x_out,
                        float* y_out, int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && W && b && out && B > 0 && n_classes > 0, "head_concat_fwd: bad arguments");
    return head_concat_fwd(x, y, W, b, out, x_out, y_out, B, n_classes, (hipStream_t)stream);
}
int gdl_head_concat_bwd(const float* x, const float* y, const float* W, const float* g_x_out, const float* g_y_out,
                        const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx, float* dy, float* dW, float* db,
                        int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && W && B > 0 && n_classes > 0, "head_concat_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dW != nullptr) == (db != nullptr),
                "head_concat_bwd: dx/dy and dW/db come in pairs");
    return head_concat_bwd(x, y, W, g_x_out, g_y_out, g_out, out_reaches_xy, uni_in_dw, dx, dy, dW, db, B, n_classes,
                           (hipStream_t)stream);
}
int gdl_head_sum_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                     float* out, float* x_out, float* y_out, int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && Wx && bx && Wy && by && out && B > 0 && n_classes > 0, "head_sum_fwd: bad arguments");
    return head_sum_fwd(x, y, Wx, bx, Wy, by, out, x_out, y_out, B, n_classes, (hipStream_t)stream);
}
int gdl_head_sum_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* g_x_out,
                     const float* g_y_out, const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx, float* dy,
                     float* dWx, float* dbx, float* dWy, float* dby, int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && Wx && Wy && B > 0 && n_classes > 0, "head_sum_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr), "head_sum_bwd: dx/dy come in pairs");
    GDL_REQUIRE((dWx != nullptr) == (dbx != nullptr) && (dWy != nullptr) == (dby != nullptr) && (dWx != nullptr) == (dWy != nullptr),
                "head_sum_bwd: dWx/dbx/dWy/dby come together");
    return head_sum_bwd(x, y, Wx, Wy, g_x_out, g_y_out, g_out, out_reaches_xy, uni_in_dw, dx, dy, dWx, dbx, dWy, dby, B,
                        n_classes, (hipStream_t)stream);
}
int gdl_head_gated_fwd(const float* x, const float* y, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* Wo, const float* bo, float* hx, float* hy, float* out, float* x_out, float* y_out, int B,
                       int n_classes, void* stream) {
    GDL_REQUIRE(x && y && W1 && b1 && W2 && b2 && Wo && bo && hx && hy && out && B > 0 && n_classes > 0,
                "head_gated_fwd: bad arguments");
    return head_gated_fwd(x, y, W1, b1, W2, b2, Wo, bo, hx, hy, out, x_out, y_out, B, n_classes, (hipStream_t)stream);
}
int gdl_head_gated_bwd(const float* x, const float* y, const float* hx, const float* hy, const float* W1, const float* W2,
                       const float* Wo, const float* g_x_out, const float* g_y_out, const float* g_out, int uni_in_dw,
                       float* dx, float* dy, float* dW1, float* db1, float* dW2, float* db2, float* dWo, float* dbo, float* ws,
                       int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && hx && hy && W1 && W2 && Wo && ws && B > 0 && n_classes > 0, "head_gated_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dWo != nullptr) == (dbo != nullptr), "head_gated_bwd: dx/dy, dWo/dbo pairs");
    GDL_REQUIRE((dW1 != nullptr) == (db1 != nullptr) && (dW1 != nullptr) == (dW2 != nullptr) && (dW1 != nullptr) == (db2 != nullptr),
                "head_gated_bwd: dW1/db1/dW2/db2 come together");
    return head_gated_bwd(x, y, hx, hy, W1, W2, Wo, g_x_out, g_y_out, g_out, uni_in_dw, dx, dy, dW1, db1, dW2, db2, dWo, dbo, ws, B,
                          n_classes, (hipStream_t)stream);
}
int gdl_head_gated_joint_fwd(const float* x, const float* y, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* Wo, const float* bo, float* hx, float* hy, float* out, int x_gate, int B, int n_classes,
                             void* stream) {
    GDL_REQUIRE(x && y && W1 && b1 && W2 && b2 && Wo && bo && hx && hy && out && B > 0 && n_classes > 0,
                "head_gated_joint_fwd: bad arguments");
    return head_gated_joint_fwd(x, y, W1, b1, W2, b2, Wo, bo, hx, hy, out, x_gate != 0, B, n_classes, (hipStream_t)stream);
}
int gdl_head_gated_joint_bwd(const float* x, const float* y, const float* hx, const float* hy, const float* W1, const float* W2,
                             const float* Wo, const float* g_out, int x_gate, float* dx, float* dy, float* dW1, float* db1,
                             float* dW2, float* db2, float* dWo, float* dbo, float* ws, int B, int n_classes, void* stream) {
    GDL_REQUIRE(x && y && hx && hy && W1 && W2 && Wo && g_out && ws && B > 0 && n_classes > 0, "head_gated_joint_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dWo != nullptr) == (dbo != nullptr), "head_gated_joint_bwd: dx/dy, dWo/dbo pairs");
    GDL_REQUIRE((dW1 != nullptr) == (db1 != nullptr) && (dW1 != nullptr) == (dW2 != nullptr) && (dW1 != nullptr) == (db2 != nullptr),
                "head_gated_joint_bwd: dW1/db1/dW2/db2 come together");
    return head_gated_joint_bwd(x, y, hx, hy, W1, W2, Wo, g_out, x_gate != 0, dx, dy, dW1, db1, dW2, db2, dWo, dbo, ws, B, n_classes,
                                (hipStream_t)stream);
}
size_t gdl_head_film_workspace_bytes(int B) { return head_film_ws_bytes(B); }
int gdl_head_film_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo, const float* bo,
                      float* hidden, float* out, float* x_out, float* y_out, int B, int n_classes, void* ws, size_t ws_bytes,
                      void* stream) {
    GDL_REQUIRE(x && y && Wfc && bfc && Wo && bo && hidden && out && n_classes > 0, "head_film_fwd: bad arguments");
    return head_film_fwd(x, y, Wfc, bfc, Wo, bo, hidden, out, x_out, y_out, B, n_classes, ws, ws_bytes, (hipStream_t)stream);
}
int gdl_head_film_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden,
                      const float* g_x_out, const float* g_y_out, const float* g_out, int uni_in_dw, float* dx, float* dy,
                      float* dWfc, float* dbfc, float* dWo, float* dbo, int B, int n_classes, void* ws, size_t ws_bytes,
                      void* stream) {
    GDL_REQUIRE(x && y && Wfc && Wo && hidden && n_classes > 0, "head_film_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dWfc != nullptr) == (dbfc != nullptr) && (dWo != nullptr) == (dbo != nullptr),
                "head_film_bwd: dx/dy, dWfc/dbfc, dWo/dbo come in pairs");
    return head_film_bwd(x, y, Wfc, Wo, hidden, g_x_out, g_y_out, g_out, uni_in_dw, dx, dy, dWfc, dbfc, dWo, dbo, B, n_classes,
                         ws, ws_bytes, (hipStream_t)stream);
}
int gdl_head_film_joint_fwd(const float* x, const float* y, const float* Wfc, const float* bfc, const float* Wo, const float* bo,
                            float* hidden, float* out, int B, int n_classes, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(x && y && Wfc && bfc && Wo && bo && hidden && out && n_classes > 0, "head_film_joint_fwd: bad arguments");
    return head_film_joint_fwd(x, y, Wfc, bfc, Wo, bo, hidden, out, B, n_classes, ws, ws_bytes, (hipStream_t)stream);
}
int gdl_head_film_joint_bwd(const float* x, const float* y, const float* Wfc, const float* Wo, const float* hidden,
                            const float* g_out, float* dx, float* dy, float* dWfc, float* dbfc, float* dWo, float* dbo, int B,
                            int n_classes, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(x && y && Wfc && Wo && hidden && g_out && n_classes > 0, "head_film_joint_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dWfc != nullptr) == (dbfc != nullptr) && (dWo != nullptr) == (dbo != nullptr),
                "head_film_joint_bwd: dx/dy, dWfc/dbfc, dWo/dbo come in pairs");
    return head_film_joint_bwd(x, y, Wfc, Wo, hidden, g_out, dx, dy, dWfc, dbfc, dWo, dbo, B, n_classes, ws, ws_bytes,
                               (hipStream_t)stream);
}
int gdl_eval_count(const float* out, const float* out_a, const float* out_v, const int64_t* labels, int B, int n_classes,
                   int64_t* num, int64_t* acc, int64_t* acc_a, int64_t* acc_v, void* stream) {
    GDL_REQUIRE(out && labels && num && acc && B > 0 && n_classes > 0, "eval_count: bad arguments");
    GDL_REQUIRE((out_a != nullptr) == (acc_a != nullptr) && (out_v != nullptr) == (acc_v != nullptr),
                "eval_count: a unimodal logit set needs its counter array and vice versa");
    return eval_count(out, out_a, out_v, labels, B, n_classes, num, acc, acc_a, acc_v, (hipStream_t)stream);
}
int gdl_logspec_frames(int n_samples, int hop) {
    if (n_samples <= 0 || hop <= 0) return 0;
    return logspec_frames(n_samples, hop);
}
int gdl_logspec(const float* wave, int B, int n_samples, int n_fft, int hop, int pad_mode, float* out, void* stream) {
    GDL_REQUIRE(wave && out && B > 0 && n_samples > 0 && hop > 0, "logspec: bad arguments");
    GDL_REQUIRE(n_fft >= 16 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, "logspec: n_fft must be a power of two in [16, 2048]");
    GDL_REQUIRE(pad_mode == GDL_PAD_CONSTANT || pad_mode == GDL_PAD_REFLECT, "logspec: pad_mode must be GDL_PAD_CONSTANT or GDL_PAD_REFLECT");
    GDL_REQUIRE(pad_mode == GDL_PAD_CONSTANT || n_samples > n_fft / 2, "logspec: reflect padding needs more than n_fft/2 samples");
    return logspec(wave, B, n_samples, n_fft, hop, pad_mode == GDL_PAD_REFLECT, out, (hipStream_t)stream);
}
int gdl_wave_logspec(const void* src, size_t src_bytes, const int64_t* desc, int B, int n_samples, int n_fft, int hop, int pad_mode,
                     int out_h, int out_w, float* wave_out, float* out, void* stream) {
    GDL_REQUIRE(src && desc && out && src_bytes > 0 && B > 0 && n_samples > 0 && hop > 0, "wave_logspec: bad arguments");
    GDL_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)desc & 7) == 0, "wave_logspec: src must be 4-byte, desc 8-byte aligned");
    GDL_REQUIRE(B <= 65535 && n_samples < INT32_MAX - 4096, "wave_logspec: at most 65535 samples of less than 2^31 - 4096 values a launch");
    GDL_REQUIRE(n_fft >= 16 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, "wave_logspec: n_fft must be a power of two in [16, 2048]");
    GDL_REQUIRE(pad_mode == GDL_PAD_CONSTANT || pad_mode == GDL_PAD_REFLECT, "wave_logspec: pad_mode must be GDL_PAD_CONSTANT or GDL_PAD_REFLECT");
    GDL_REQUIRE(pad_mode == GDL_PAD_CONSTANT || n_samples > n_fft / 2, "wave_logspec: reflect padding needs more than n_fft/2 samples");
    GDL_REQUIRE(out_h >= 0 && out_w >= 0 && (out_h == 0) == (out_w == 0),
                "wave_logspec: output size %d x %d must be 0 x 0 (the spectrogram as it is) or positive", out_h, out_w);
    GDL_REQUIRE((int64_t)out_h * out_w < (int64_t)1 << 31, "wave_logspec: output size %d x %d is too large", out_h, out_w);
    return wave_logspec(src, src_bytes, (const long long*)desc, B, n_samples, n_fft, hop, pad_mode == GDL_PAD_REFLECT, out_h, out_w,
                        wave_out, out, (hipStream_t)stream);
}
int gdl_frames_normalize(const uint8_t* frames, int64_t n_img, int H, int W, const float* mean, const float* std, float* out,
                         void* stream) {
    GDL_REQUIRE(frames && out && mean && std && n_img > 0 && H > 0 && W > 0, "frames_normalize: bad arguments");
    GDL_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "frames_normalize: zero std");
    return frames_normalize(frames, (size_t)n_img, H, W, mean, std, out, (hipStream_t)stream);
}
int gdl_frames_resized_crop_box_ok(int box_h, int box_w, int out_h, int out_w) { return resized_crop_box_ok(box_h, box_w, out_h, out_w); }
int gdl_frames_resized_crop(const uint8_t* src, size_t src_bytes, const int64_t* desc, int n_img, int B, int T, int out_h, int out_w,
                            const float* mean, const float* std, float* out, void* stream) {
    GDL_REQUIRE(src && desc && out && mean && std && src_bytes > 0, "frames_resized_crop: bad arguments");
    GDL_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)desc & 7) == 0, "frames_resized_crop: src must be 4-byte, desc 8-byte aligned");
    GDL_REQUIRE(n_img > 0 && B > 0 && T > 0 && (int64_t)B * T == n_img, "frames_resized_crop: n_img (%d) must be B * T (%d * %d)", n_img, B, T);
    GDL_REQUIRE(out_h > 0 && out_w > 0, "frames_resized_crop: output size %d x %d must be positive", out_h, out_w);
    GDL_REQUIRE(resized_crop_box_ok(1, 1, out_h, out_w), "frames_resized_crop: output size %d x %d does not fit the kernel's tables", out_h, out_w);
    GDL_REQUIRE((int64_t)n_img * ((out_h + 15) / 16) < (int64_t)1 << 31, "frames_resized_crop: too many images for one launch");
    GDL_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "frames_resized_crop: zero std");
    return frames_resized_crop(src, src_bytes, (const long long*)desc, n_img, T, out_h, out_w, mean, std, out, (hipStream_t)stream);
}
int gdl_loader_plan(const int64_t* clips, const int64_t* frames, const int64_t* labels, int64_t N, int T, uint64_t seed, int64_t epoch,
                    int64_t first, int64_t count, int shuffle, int augment, int64_t n_samples, int64_t start_high, int out_h,
                    int out_w, const double* draw, int64_t* index, int64_t* label, int64_t* wave_desc, int64_t* crop_desc,
                    void* stream) {
    GDL_REQUIRE(clips && frames && labels && draw && index && label && wave_desc && crop_desc, "loader_plan: bad arguments");
    GDL_REQUIRE((((uintptr_t)clips | (uintptr_t)frames | (uintptr_t)labels | (uintptr_t)index | (uintptr_t)label |
                  (uintptr_t)wave_desc | (uintptr_t)crop_desc) & 7) == 0, "loader_plan: the tables must be 8-byte aligned");
    GDL_REQUIRE(N >= 1 && N <= INT32_MAX && T >= 1 && T <= 64, "loader_plan: N (%lld) must be in [1, 2^31 - 1] and T (%d) in [1, 64]",
                (long long)N, T);
    GDL_REQUIRE(first >= 0 && count >= 1 && first <= N && count <= N - first,
                "loader_plan: positions [%lld, %lld + %lld) do not lie inside an epoch of %lld", (long long)first, (long long)first,
                (long long)count, (long long)N);
    GDL_REQUIRE((shuffle == 0 || shuffle == 1) && (augment == 0 || augment == 1), "loader_plan: shuffle and augment are 0 or 1");
    GDL_REQUIRE(n_samples >= 1 && start_high >= 0 && n_samples < INT32_MAX - 4096 && start_high < INT32_MAX - n_samples,
                "loader_plan: a window of %lld samples starting at up to %lld does not fit 2^31", (long long)n_samples, (long long)start_high);
    GDL_REQUIRE(out_h > 0 && out_w > 0 && resized_crop_box_ok(1, 1, out_h, out_w),
                "loader_plan: output size %d x %d does not fit the resize kernel's tables", out_h, out_w);
    const LoaderDraw dr{draw[0], draw[1], draw[2], draw[3], draw[4], draw[5], draw[6]};
    GDL_REQUIRE(dr.scale_lo > 0 && dr.scale_lo <= dr.scale_hi && dr.scale_hi < 1e6 && dr.ratio_lo > 0 && dr.ratio_lo <= dr.ratio_hi &&
                    dr.ratio_hi < 1e6 && dr.log_ratio_lo <= dr.log_ratio_hi && dr.log_ratio_lo > -50 && dr.log_ratio_hi < 50 &&
                    dr.p_flip >= 0 && dr.p_flip <= 1,
                "loader_plan: draw = {scale_lo, scale_hi, ratio_lo, ratio_hi, log ratio_lo, log ratio_hi, p_flip} out of range");
    return loader_plan((const long long*)clips, (const long long*)frames, (const long long*)labels, N, T, seed, epoch, first, count,
                       shuffle, augment, start_high, dr, (long long*)index, (long long*)label, (long long*)wave_desc,
                       (long long*)crop_desc, (hipStream_t)stream);
}
int gdl_softmax_ce3(const float* logits0, const float* logits1, const float* logits2, const int64_t* labels, float scale0,
                    float scale1, float scale2, float* losses, float* dlogits0, float* dlogits1, float* dlogits2, int B,
                    int n_classes, void* stream) {
    GDL_REQUIRE(logits0 && logits1 && logits2 && labels && losses && B > 0 && n_classes > 0, "softmax_ce3: bad arguments");
    const float* lg[3] = {logits0, logits1, logits2};
    float* dl[3] = {dlogits0, dlogits1, dlogits2};
    const float sc[3] = {scale0, scale1, scale2};
    return softmax_ce_multi(3, lg, labels, sc, losses, dl, B, n_classes, (hipStream_t)stream);
}
int gdl_softmax_ce(const float* logits, const int64_t* labels, float scale, float* loss, float* dlogits, int B,
                   int n_classes, void* stream) {
    GDL_REQUIRE(logits && labels && loss && B > 0 && n_classes > 0, "softmax_ce: bad arguments");
    return softmax_ce(logits, labels, scale, loss, dlogits, B, n_classes, (hipStream_t)stream);
}

int gdl_head_concat_xy_fwd(const float* x, const float* y, const float* W, const float* b, float* out, float* x_out, float* y_out,
                           int B, int n_classes, int x_dim, int y_dim, void* stream) {
    GDL_REQUIRE(x && y && W && b && out && B > 0 && n_classes > 0 && x_dim > 0 && y_dim > 0, "head_concat_xy_fwd: bad arguments");
    return head_concat_xy_fwd(x, y, W, b, out, x_out, y_out, B, n_classes, x_dim, y_dim, (hipStream_t)stream);
}
int gdl_head_concat_xy_bwd(const float* x, const float* y, const float* W, const float* g_x_out, const float* g_y_out,
                           const float* g_out, int out_reaches_xy, int uni_in_dw, float* dx, float* dy, float* dW, float* db, int B,
                           int n_classes, int x_dim, int y_dim, void* stream) {
    GDL_REQUIRE(x && y && W && B > 0 && n_classes > 0 && x_dim > 0 && y_dim > 0, "head_concat_xy_bwd: bad arguments");
    GDL_REQUIRE((dx != nullptr) == (dy != nullptr) && (dW != nullptr) == (db != nullptr), "head_concat_xy_bwd: dx/dy and dW/db come in pairs");
    return head_concat_xy_bwd(x, y, W, g_x_out, g_y_out, g_out, out_reaches_xy, uni_in_dw, dx, dy, dW, db, B, n_classes, x_dim, y_dim,
                              (hipStream_t)stream);
}
// ---- Swin visual encoder: non-GEMM operators; the Linears are gdl_conv_fwd / _dgrad / _wgrad (1x1)
int gdl_swin_patch_gather(int dtype, const float* x, void* a, int B, int T, int H, int W, int patch, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && a, "swin_patch_gather: bad arguments");
    return swin_patch_gather(dtype, x, a, B, T, H, W, patch, (hipStream_t)stream);
}
int gdl_swin_bias_act(int dtype, void* y, const float* bias, void* u, const void* res, size_t M, int ld, int mode, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && y && bias, "swin_bias_act: bad arguments");
    return swin_bias_act(dtype, y, bias, u, res, M, ld, mode, (hipStream_t)stream);
}
int gdl_linear_bwd_ok(int dtype, size_t M, int K, int N) { return linear_bwd_ok(dtype, M, K, N) ? 1 : 0; }
size_t gdl_linear_bwd_workspace_bytes(size_t M, int K, int N) { return linear_bwd_ok(GDL_BF16, M, K, N) ? linear_bwd_ws_bytes(M, K, N) : 0; }
int gdl_linear_bwd(int dtype, const void* dy, const void* x, const void* wT, void* dx, float* dw, float* db, void* ws, size_t ws_bytes,
                   size_t M, int K, int Kreal, int N, void* stream) {
    GDL_REQUIRE(dtype == GDL_BF16, "linear_bwd: bf16 only");
    return linear_bwd(dy, x, wT, dx, dw, db, ws, ws_bytes, M, K, Kreal, N, (hipStream_t)stream);
}
int gdl_swin_drop_path(int dtype, const void* y, const void* res, const float* scale, void* out, size_t M, int L, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype), "swin_drop_path: bad dtype");
    return swin_drop_path(dtype, y, res, scale, out, M, L, ld, (hipStream_t)stream);
}
int gdl_swin_ln_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats, size_t M, int C, int ld,
                    void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && gamma && beta && y && stats, "swin_ln_fwd: bad arguments");
    return swin_ln_fwd(dtype, x, gamma, beta, y, stats, M, C, ld, (hipStream_t)stream);
}
size_t gdl_swin_partial_bytes(int ld) { return swin_partial_bytes(ld); }
int gdl_swin_ln_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, const void* add, void* dx,
                    float* dgamma_dbeta, void* partial, size_t M, int C, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && x && stats && gamma && dx, "swin_ln_bwd: bad arguments");
    return swin_ln_bwd(dtype, dy, x, stats, gamma, add, dx, dgamma_dbeta, (float*)partial, M, C, ld, (hipStream_t)stream);
}
int gdl_swin_ln_bwd_colsum(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, const void* add,
                           void* dx, float* dgamma_dbeta_colsum, void* partial, size_t M, int C, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && x && stats && gamma && dx, "swin_ln_bwd_colsum: bad arguments");
    return swin_ln_bwd(dtype, dy, x, stats, gamma, add, dx, dgamma_dbeta_colsum, (float*)partial, M, C, ld, (hipStream_t)stream, true);
}
int gdl_swin_colsum(int dtype, void* g, const void* u, float* db, void* partial, size_t M, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && g, "swin_colsum: bad arguments");
    return swin_colsum(dtype, g, u, db, (float*)partial, M, ld, (hipStream_t)stream);
}
int gdl_swin_attn_fwd(int dtype, const void* qkv, const float* table, void* out, int n_img, int H, int W, int window, int shift,
                      int heads, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && qkv && table && out, "swin_attn_fwd: bad arguments");
    return swin_attn_fwd(dtype, qkv, table, out, n_img, H, W, window, shift, heads, ld, (hipStream_t)stream);
}
size_t gdl_swin_attn_bwd_workspace_bytes(int n_img, int H, int W, int window, int heads) {
    if (window <= 0) return 0;
    const size_t general = swin_attn_bwd_ws_bytes(n_img, (H / window) * (W / window), window, heads);
    const size_t seven = window == 7 ? swin_attn7_bwd_ws_bytes(n_img, H, W, heads) : 0;  // either kernel may serve the call
    return general > seven ? general : seven;
}
int gdl_swin_attn_bwd(int dtype, const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable, void* ws, int n_img,
                      int H, int W, int window, int shift, int heads, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && qkv && table && dout && dqkv, "swin_attn_bwd: bad arguments");
    return swin_attn_bwd(dtype, qkv, table, dout, dqkv, dtable, (float*)ws, n_img, H, W, window, shift, heads, ld, (hipStream_t)stream);
}
int gdl_swin_merge(int dtype, const void* src, void* dst, int N, int H, int W, int C, int ldx, int scatter, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && src && dst, "swin_merge: bad arguments");
    return swin_merge(dtype, src, dst, N, H, W, C, ldx, scatter, (hipStream_t)stream);
}
int gdl_swin_token_mean(int dtype, const void* x, float* y, int N, int L, int C, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && x && y, "swin_token_mean: bad arguments");
    return swin_token_mean(dtype, x, y, N, L, C, ld, (hipStream_t)stream);
}
int gdl_swin_token_mean_bwd(int dtype, const float* dy, void* dx, int N, int L, int C, int ld, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && dy && dx, "swin_token_mean_bwd: bad arguments");
    return swin_token_mean_bwd(dtype, dy, dx, N, L, C, ld, (hipStream_t)stream);
}
int gdl_swin_pack_matrix(int dtype, const float* src, void* dst, void* dstT, int n, int k, int nseg, int nseg_pad, int kseg,
                         int kseg_pad, void* stream) {
    GDL_REQUIRE(dt_ok(dtype) && src && dst, "swin_pack_matrix: bad arguments");
    return swin_pack_matrix(dtype, src, dst, dstT, n, k, nseg, nseg_pad, kseg, kseg_pad, (hipStream_t)stream);
}
int gdl_swin_ln_bwd_rows(int dtype, size_t M, int ld) {
    if (!dt_ok(dtype) || ld <= 0 || ld % 64 != 0 || M == 0) return 0;  // (a count, not a status: 0 = bad arguments)
    return swin_ln_bwd_rows(dtype, M, ld);
}
int gdl_swin_colsum_rows(int dtype, size_t M, int ld) {
    if (!dt_ok(dtype) || ld <= 0 || ld % 64 != 0 || M == 0) return 0;
    return swin_colsum_rows(dtype, M, ld);
}
int gdl_swin_partial_reduce_batched(const void* descs, int n_desc, int total_blocks, void* stream) {
    return swin_partial_reduce_batched(descs, n_desc, total_blocks, (hipStream_t)stream);
}
int gdl_swin_pack_batched(const void* descs, int n_desc, int total_blocks, int dir, void* stream) {
    return swin_pack_batched(descs, n_desc, total_blocks, dir, (hipStream_t)stream);
}
int gdl_swin_unpack_matrix(const float* src, float* dst, int n, int k, int nseg, int nseg_pad, int kseg, int kseg_pad, void* stream) {
    GDL_REQUIRE(src && dst, "swin_unpack_matrix: null pointer");
    return swin_unpack_matrix(src, dst, n, k, nseg, nseg_pad, kseg, kseg_pad, (hipStream_t)stream);
}

}  // extern "C"
