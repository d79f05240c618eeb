// head_cls.hip -- the classifier of the unimodal baselines, float32.
//
// AVClassifier_DGL with modality 'audio' / 'visual' (the reference's models/basic_model.py:46-59, 88-122) puts one
// nn.Linear(512, n_classes) on the pooled features of its only encoder; main.py trains it with one CrossEntropyLoss.
//   out = f W^T + b;   loss = mean CE(out, labels);   dlogits = scale * (softmax(out) - onehot) / B
//   df = dlogits W;    dW = dlogits^T f;    db = sum_b dlogits
// Three entry points: the forward (eval, the drop-in module), the backward for an arbitrary upstream gradient (the drop-in
// module; the step's parameter gradients with df = NULL), and head_cls_ce, the ONE launch that stands between the encoder's
// forward and its backward in the training step (logits, loss, dlogits and df), where head_uni_dfeat_kernel stands in the
// DGL step.  Sizes are tiny (B x 512 x n): latency bound, no MFMA.
//
// Every sum has ONE order, shared by the three launchers through the device functions of head_body.h, so head_cls_ce's out,
// dlogits and df carry the bits of head_cls_fwd + softmax_ce (head.hip) + head_cls_bwd (the orders: head_body.h; dW / db:
// samples in ascending order).
#include <map>
#include <mutex>
#include <utility>

#include "common.h"
#include "head_body.h"
#include "ops.h"
#include "prof.h"
#include "ticket.h"

namespace gdl {

constexpr int CLS_D = 512;   // feature width
constexpr int CLS_ND = 8;    // features per lane
constexpr int CLS_MAXN = HB_MAXN;

// ---------------------------------------------------------------- forward
// grid = (B, ceil(n / 8)): a block's four waves own eight classes of one sample, two per wave
constexpr int CLS_FWD_CH = 8;
__global__ __launch_bounds__(256) void head_cls_fwd_kernel(const float* __restrict__ f, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ out, int n) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.y * CLS_FWD_CH + wave, j2 = j + 4;
    if (j >= n) return;
    float fv[CLS_ND];
    head_load_feat<CLS_ND>(f + (size_t)b * CLS_D, lane, fv);
    float pa, pb;
    head_dot2<CLS_ND>(W + (size_t)j * CLS_D, W + (size_t)(j2 < n ? j2 : j) * CLS_D, fv, lane, pa, pb);
    if (lane == 0) {
        out[(size_t)b * n + j] = pa + bias[j];
        if (j2 < n) out[(size_t)b * n + j2] = pb + bias[j2];
    }
}
int head_cls_fwd(const float* f, const float* W, const float* b, float* out, int B, int n, hipStream_t st) {
    GDL_REQUIRE(n <= CLS_MAXN, "head_cls_fwd: at most %d classes", CLS_MAXN);
    hipLaunchKernelGGL(head_cls_fwd_kernel, dim3(B, ceil_div(n, CLS_FWD_CH)), dim3(256), 0, st, f, W, b, out, n);
    GDL_CHECK_LAUNCH("head_cls_fwd_kernel");
    return GDL_OK;
}

// ---------------------------------------------------------------- backward for an arbitrary upstream gradient
// grid = (B, 2): a thread per feature, the sample's class gradients staged in LDS once
__global__ __launch_bounds__(256) void head_cls_dfeat_kernel(const float* __restrict__ W, const float* __restrict__ g_out,
                                                             float* __restrict__ df, int n) {
    __shared__ float g[CLS_MAXN];
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += 256) g[j] = g_out[(size_t)b * n + j];
    __syncthreads();
    const int i = blockIdx.y * 256 + threadIdx.x;
    df[(size_t)b * CLS_D + i] = head_df_walk(g, W, CLS_D, i, n);
}
// grid = (n, 2): a thread per weight-gradient element; the batch's gradients of class j staged in LDS 256 samples at a time,
// summed in sample order; db[j] = their plain sum in the same order (the y = 0 block)
__global__ __launch_bounds__(256) void head_cls_dw_kernel(const float* __restrict__ f, const float* __restrict__ g_out,
                                                          float* __restrict__ dW, float* __restrict__ db, int B, int n) {
    __shared__ float gs[256];
    const int j = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    float s = 0.f, sb = 0.f;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int nb = min(256, B - b0);
        __syncthreads();
        if ((int)threadIdx.x < nb) gs[threadIdx.x] = g_out[(size_t)(b0 + threadIdx.x) * n + j];
        __syncthreads();
#pragma unroll 8
        for (int b = 0; b < nb; ++b) {
            s = fmaf(gs[b], f[(size_t)(b0 + b) * CLS_D + i], s);
            sb += gs[b];
        }
    }
    if (dW) dW[(size_t)j * CLS_D + i] = s;
    if (db && blockIdx.y == 0 && threadIdx.x == 0) db[j] = sb;
}
static_assert(CLS_D == 2 * 256, "head_cls_dfeat_kernel / head_cls_dw_kernel: two blocks of 256 features");
int head_cls_bwd(const float* f, const float* W, const float* g_out, float* df, float* dW, float* db, int B, int n,
                 hipStream_t st) {
    GDL_REQUIRE(n <= CLS_MAXN, "head_cls_bwd: at most %d classes", CLS_MAXN);
    if (df) {
        hipLaunchKernelGGL(head_cls_dfeat_kernel, dim3(B, 2), dim3(256), 0, st, W, g_out, df, n);
        GDL_CHECK_LAUNCH("head_cls_dfeat_kernel");
    }
    if (dW || db) {
        // (db alone: the y = 0 blocks; they still walk the features of their half, B x 256 fmaf each -- never on a hot path)
        hipLaunchKernelGGL(head_cls_dw_kernel, dim3(n, dW ? 2 : 1), dim3(256), 0, st, f, g_out, dW, db, B, n);
        GDL_CHECK_LAUNCH("head_cls_dw_kernel");
    }
    return GDL_OK;
}

// ---------------------------------------------------------------- the training step's launch
// grid = B, 16 waves per sample: head_ce_body (head_body.h; head_uni_dfeat_kernel<8> in the DGL step is the same body) plus the
// three stores the unimodal step needs -- out and dlogits (the body's STORE) and the sample's loss term.
//
// The mean over the samples = over the blocks.  df occupies waves 0 .. 7 only; wave 15, idle by then, publishes the sample's
// term (lse - logit[label]) and draws a ticket (ticket.h: the protocol and its visibility argument); the block whose ticket is
// the last sums all B terms in ONE order of this kernel's own (lane l takes b = l, l + 64, ..., then the xor butterfly
// 32 .. 1), writes loss[0] and hands the counter back.  `part` / `cnt` belong to the launching stream (ce_slot below).
__global__ __launch_bounds__(1024) void head_cls_ce_kernel(const float* __restrict__ f, const float* __restrict__ W,
                                                          const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                          float scale, float* __restrict__ out, float* __restrict__ loss,
                                                          float* __restrict__ dlogits, float* __restrict__ df,
                                                          float* __restrict__ part, unsigned* __restrict__ cnt, int B, int n) {
    __shared__ HeadBodyLds s;
    const int lab = head_ce_body<CLS_ND, true>(s, f, W, CLS_D, bias, labels, scale, out, dlogits, df, B, n);
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == HB_NW - 1) {  // (beyond the df walk's threads)
        int last = 0;
        if (lane == 0) {
            st_agent(part + b, lab >= 0 ? s.lse - s.lg[lab] : __builtin_nanf(""));
            last = ticket_draw(cnt, B);
        }
        last = __shfl(last, 0);
        if (last) {
            float t = 0.f;
            for (int k = lane; k < B; k += 64) t += ld_agent(part + k);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) {
                loss[0] = t / (float)B;
                ticket_hand_back(cnt);
            }
        }
    }
}

// The ticket counter and the B loss terms of a launch in flight: device memory owned by the library, one slot per (device,
// stream), made at the first call on that stream (the only time this launcher allocates, zeroes and thereby synchronises) and
// grown when a larger batch comes.  Launches on one stream run one after the other, launches on different streams use
// different slots: no two kernels in flight share a counter.
namespace {
struct CeSlot {
    float* base = nullptr;  // [0]: the counter, on a 256-byte line of its own; [64 ..): the terms
    int cap = 0;
};
std::mutex ce_mu;
std::map<std::pair<int, hipStream_t>, CeSlot> ce_slots;
}  // namespace
static int ce_slot(hipStream_t st, int B, float** part, unsigned** cnt) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return check_hip(hipGetLastError(), "head_cls_ce: hipGetDevice");
    std::lock_guard<std::mutex> lock(ce_mu);
    CeSlot& s = ce_slots[{dev, st}];
    if (s.cap < B) {
        if (s.base) {
            hipError_t e = hipFree(s.base);  // (waits for the device: the slot's last launch is done)
            s.base = nullptr, s.cap = 0;
            if (e != hipSuccess) return check_hip(e, "head_cls_ce: hipFree");
        }
        const int cap = (int)align_up((size_t)B, 1024);
        float* p = nullptr;
        hipError_t e = hipMalloc((void**)&p, (64 + (size_t)cap) * sizeof(float));
        if (e != hipSuccess) return check_hip(e, "head_cls_ce: hipMalloc");
        e = hipMemset(p, 0, (64 + (size_t)cap) * sizeof(float));
        if (e != hipSuccess) {
            (void)hipFree(p);
            return check_hip(e, "head_cls_ce: hipMemset");
        }
        s.base = p, s.cap = cap;
    }
    *cnt = (unsigned*)s.base;
    *part = s.base + 64;
    return GDL_OK;
}
int head_cls_ce(const float* f, const float* W, const float* b, const int64_t* labels, float scale, float* out, float* loss,
                float* dlogits, float* df, int B, int n, hipStream_t st) {
    GDL_REQUIRE(n <= CLS_MAXN, "head_cls_ce: at most %d classes", CLS_MAXN);
    float* part = nullptr;
    unsigned* cnt = nullptr;
    const int rc = ce_slot(st, B, &part, &cnt);
    if (rc != GDL_OK) return rc;
    ProfScope prof("gdl::head_cls_ce_kernel", PROF_HBM, st, (double)B * CLS_D * 8.0 + (double)n * CLS_D * 4.0 + (double)B * n * 8.0);
    hipLaunchKernelGGL(head_cls_ce_kernel, dim3(B), dim3(1024), 0, st, f, W, b, labels, scale, out, loss, dlogits, df, part, cnt, B, n);
    GDL_CHECK_LAUNCH("head_cls_ce_kernel");
    return GDL_OK;
}

}  // namespace gdl
