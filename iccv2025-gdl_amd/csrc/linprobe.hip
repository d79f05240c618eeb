// linprobe.hip -- the linear probe of a frozen encoder: a whole epoch of main.py's unimodal step with the encoder removed, on
// features that already sit on the device (gdl.extract_features' bank), behind ONE C call.
//
// Per step, for the B bank rows the step's slice of the order table names (f = bank[order[s][b]], y = labels[order[s][b]]):
//   out = f W^T + b;  loss = mean CE(out, y);  dlogits = (softmax(out) - onehot) / B;  dW = dlogits^T f;  db = sum_b dlogits
//   clip_grad_norm_({dW, db}, max_norm):  norm in double, coef = min(1, max_norm / (norm + 1e-6))         (optim.hip's)
//   optim.SGD:  d = coef g + wd p;  m = mu m + d;  p -= lr m                                                 (optim.hip's)
// THREE launches per step, chained by stream order alone -- no block ever waits for or hands data to another block inside a
// launch, so there is no ticket, no counter and nothing to re-zero (the choice against a two-launch form whose last block
// clips and updates alone: profiles/probe_bench.txt):
//   linprobe_ce_kernel      grid B x 1024: head_ce_logits (head_body.h) on the gathered row -- the logits, the softmax and the
//                           logit gradient carry the bits of gdl_head_cls_ce on the same rows -- and the sample's loss term
//   linprobe_dw_kernel      grid (n, 2) x 256: a thread per element of dW, samples in ascending order (head_cls_dw_kernel's
//                           order, on gathered rows), db[j] beside it, and the block's sum of squares in double
//   linprobe_update_kernel  grid ceil(n / 2) x 256: every block adds the 2 n block sums in the same order (so all hold the same
//                           coefficient), then clips and updates its own 256 float4 of W / mW; block 0 also takes b / mb and
//                           adds the step's mean loss to loss_acc
// Every sum has ONE order and there is no floating-point atomic: two epochs from the same state and order table are
// bit-identical.  The loss sum is softmax_ce_block's (head.hip): 256 partial sums p[b & 255] taking b, b + 256, ... in turn,
// then the tree p[i] += p[i + o], o = 128 .. 1.
#include "common.h"
#include "head_body.h"
#include "ops.h"

namespace gdl {

constexpr int LP_D = 512;  // feature width
constexpr int LP_ND = 8;   // features per lane
constexpr int LP_NT = 256;

// a row of the bank: an index outside [0, N) reads row 0 (never outside the bank) and is reported through `ok`
__device__ __forceinline__ size_t lp_row(const int32_t* __restrict__ order, int b, int64_t N, bool& ok) {
    const int64_t r = (int64_t)order[b];
    ok = r >= 0 && r < N;
    return ok ? (size_t)r : (size_t)0;
}

__global__ __launch_bounds__(1024) void linprobe_ce_kernel(const float* __restrict__ bank, const int64_t* __restrict__ labels,
                                                          int64_t N, const int32_t* __restrict__ order,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          float* __restrict__ dlogits, float* __restrict__ part, int B, int n) {
    __shared__ HeadBodyLds s;
    const int b = blockIdx.x;
    bool ok;
    const size_t row = lp_row(order, b, N, ok);
    const int lab = head_ce_logits<LP_ND, false>(s, bank + row * LP_D, W, LP_D, bias, labels + row, 1.f, nullptr, nullptr, B, n);
    for (int j = threadIdx.x; j < n; j += 1024) dlogits[(size_t)b * n + j] = s.dl[j];
    if (threadIdx.x == 0) part[b] = (ok && lab >= 0) ? s.lse - s.lg[lab] : __builtin_nanf("");
}

// partial[2 j + y]: the sum of squares of dW[j][256 y .. 256 y + 255] (+ db[j]^2 at y = 0): each square exact in double, the
// 256 of them folded by the tree i += i + o, o = 128 .. 1
__global__ __launch_bounds__(LP_NT) void linprobe_dw_kernel(const float* __restrict__ bank, int64_t N,
                                                           const int32_t* __restrict__ order, const float* __restrict__ dlogits,
                                                           float* __restrict__ dW, float* __restrict__ db,
                                                           double* __restrict__ partial, int B, int n) {
    __shared__ float gs[LP_NT];
    __shared__ size_t rows[LP_NT];
    __shared__ double sh[LP_NT];
    const int j = blockIdx.x, t = threadIdx.x, i = blockIdx.y * LP_NT + t;
    float s = 0.f, sb = 0.f;
    for (int b0 = 0; b0 < B; b0 += LP_NT) {
        const int nb = min(LP_NT, B - b0);
        __syncthreads();
        if (t < nb) {
            bool ok;
            gs[t] = dlogits[(size_t)(b0 + t) * n + j];
            rows[t] = lp_row(order, b0 + t, N, ok) * LP_D;
        }
        __syncthreads();
#pragma unroll 8
        for (int b = 0; b < nb; ++b) {
            s = fmaf(gs[b], bank[rows[b] + i], s);
            sb += gs[b];
        }
    }
    dW[(size_t)j * LP_D + i] = s;
    double q = (double)s * (double)s;
    if (blockIdx.y == 0 && t == 0) {
        db[j] = sb;
        q += (double)sb * (double)sb;
    }
    sh[t] = q;
    __syncthreads();
    for (int o = LP_NT / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) partial[2 * j + blockIdx.y] = sh[0];
}
static_assert(LP_D == 2 * LP_NT, "linprobe_dw_kernel: two blocks of 256 features per class");

// d = g k + wd p; m = mu m + d; p -= lr m -- sgd_kernel's (optim.hip) spelling
__device__ __forceinline__ void lp_sgd1(float& p, float g, float& m, float k, float lr, float mu, float wd) {
    m = mu * m + (g * k + wd * p);
    p -= lr * m;
}

__global__ __launch_bounds__(LP_NT) void linprobe_update_kernel(float* __restrict__ W, float* __restrict__ bias,
                                                               float* __restrict__ mW, float* __restrict__ mb,
                                                               const float* __restrict__ dW, const float* __restrict__ db,
                                                               const double* __restrict__ partial, const float* __restrict__ part,
                                                               double* __restrict__ loss_acc, float lr, float mu, float wd,
                                                               float max_norm, int B, int n) {
    __shared__ double sh[LP_NT];
    __shared__ float lsh[LP_NT];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int k = t; k < 2 * n; k += LP_NT) a += partial[k];
    sh[t] = a;
    __syncthreads();
    for (int o = LP_NT / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const double norm = sqrt(sh[0]);
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    const float k = (float)coef;
    const int q = blockIdx.x * LP_NT + t;
    if (q < n * (LP_D / 4)) {
        float4 pv = ((float4*)W)[q], mv = ((float4*)mW)[q];
        const float4 gv = ((const float4*)dW)[q];
        lp_sgd1(pv.x, gv.x, mv.x, k, lr, mu, wd);
        lp_sgd1(pv.y, gv.y, mv.y, k, lr, mu, wd);
        lp_sgd1(pv.z, gv.z, mv.z, k, lr, mu, wd);
        lp_sgd1(pv.w, gv.w, mv.w, k, lr, mu, wd);
        ((float4*)mW)[q] = mv;
        ((float4*)W)[q] = pv;
    }
    if (blockIdx.x != 0) return;
    for (int j = t; j < n; j += LP_NT) {
        float p = bias[j], m = mb[j];
        lp_sgd1(p, db[j], m, k, lr, mu, wd);
        mb[j] = m;
        bias[j] = p;
    }
    float ls = 0.f;
    for (int b = t; b < B; b += LP_NT) ls += part[b];
    lsh[t] = ls;
    __syncthreads();
    for (int o = LP_NT / 2; o > 0; o >>= 1) {
        if (t < o) lsh[t] += lsh[t + o];
        __syncthreads();
    }
    if (t == 0) {  // (launches on one stream are ordered: the single writer of loss_acc)
        loss_acc[0] += (double)(lsh[0] / (float)B);
        loss_acc[1] += 1.0;
    }
}

// ws: [dlogits B n | loss terms B | dW n 512 | db n | block sums 2 n (double)], each part on a 256-byte boundary
namespace {
struct LpLayout {
    size_t part, dW, db, partial, total;
};
LpLayout lp_layout(int B, int n) {
    LpLayout l;
    l.part = align_up((size_t)B * n * sizeof(float), 256);
    l.dW = l.part + align_up((size_t)B * sizeof(float), 256);
    l.db = l.dW + (size_t)n * LP_D * sizeof(float);
    l.partial = l.db + align_up((size_t)n * sizeof(float), 256);
    l.total = l.partial + align_up((size_t)2 * n * sizeof(double), 256);
    return l;
}
}  // namespace

size_t linprobe_ws_bytes(int B, int n) { return (B < 1 || n < 1 || n > HB_MAXN) ? 0 : lp_layout(B, n).total; }

int linprobe_epoch(const float* bank, const int64_t* labels, int64_t N, const int32_t* order, int steps, int B, float* W, float* b,
                   float* mW, float* mb, int n, float lr, float mu, float wd, float max_norm, double* loss_acc, void* ws,
                   hipStream_t st) {
    const LpLayout l = lp_layout(B, n);
    unsigned char* w = (unsigned char*)ws;
    float* dlogits = (float*)w;
    float* part = (float*)(w + l.part);
    float* dW = (float*)(w + l.dW);
    float* db = (float*)(w + l.db);
    double* partial = (double*)(w + l.partial);
    for (int s = 0; s < steps; ++s) {
        const int32_t* ord = order + (size_t)s * B;
        hipLaunchKernelGGL(linprobe_ce_kernel, dim3(B), dim3(1024), 0, st, bank, labels, N, ord, (const float*)W, (const float*)b,
                           dlogits, part, B, n);
        GDL_CHECK_LAUNCH("linprobe_ce_kernel");
        hipLaunchKernelGGL(linprobe_dw_kernel, dim3(n, 2), dim3(LP_NT), 0, st, bank, N, ord, (const float*)dlogits, dW, db,
                           partial, B, n);
        GDL_CHECK_LAUNCH("linprobe_dw_kernel");
        hipLaunchKernelGGL(linprobe_update_kernel, dim3(ceil_div(n * (LP_D / 4), LP_NT)), dim3(LP_NT), 0, st, W, b, mW, mb,
                           (const float*)dW, (const float*)db, (const double*)partial, (const float*)part, loss_acc, lr, mu, wd,
                           max_norm, B, n);
        GDL_CHECK_LAUNCH("linprobe_update_kernel");
    }
    return GDL_OK;
}

}  // namespace gdl
