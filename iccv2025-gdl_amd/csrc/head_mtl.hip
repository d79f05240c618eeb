// head_mtl.hip -- the junction of the step whose fused loss reaches the encoders (DGLTrainer, detach_fused=False: the DGL
// ablation "no detach" and the multi-task baseline loss_f + gamma (loss_a + loss_v), main.py:177), float32.
//
// The concat / sum DGL head without its .detach() (fusion_modules.py:16-30, 45-59):
//   out_a = fa Wa^T + ba,  out_v = fv Wv^T + bv,  out = fa Wa^T + fv Wv^T + (ba [+ bv])
//   losses = {CE(out), CE(out_a), CE(out_v)};  g_f = dCE(out), g_a = scale_u dCE(out_a), g_v = scale_u dCE(out_v)
//   dfa = (g_a + fused_reaches g_f) Wa,  dfv = (g_v + fused_reaches g_f) Wv
// An encoder's feature gradient now needs BOTH encoders' features, so the early-backward form of the DGL step does not apply and
// head_fwd + softmax_ce3 + head_bwd_feat (head.hip) would stand between the two forwards and the two backward chains: three
// launches on the critical path.  This is the ONE launch that replaces them there, as head_uni_dfeat_kernel does for the DGL
// step and head_cls_ce_kernel for the unimodal one.
//
// Every sum has the order and the spelling of head_body.h (= of the three launches): the two 512-dots of a class are taken once
// and serve all three logit sets (out = pa + pv + bias); softmax as in head_ce_body, three sets side by side (their serial
// exp-sums on three different waves) -- a text of its own: on head_ce_logits made a template over the number of sets this kernel
// needs 2 KiB more LDS and measures 0.1 - 0.2 us slower at 64 x 309 (docs/measurement_log.md), so both are kept; g_a + g_f added before the walk; classes ascending in the walk.  The logits, the logit
// gradients and dfa / dfv carry the bits of the three-launch path.
#include "common.h"
#include "head_body.h"
#include "ops.h"
#include "prof.h"
#include "ticket.h"

namespace gdl {

constexpr int MTL_D = 512;  // features per modality
constexpr int MTL_ND = 8;   // features per lane
static_assert(2 * MTL_D == 64 * HB_NW, "head_mtl_ce_kernel: a thread per element of [dfa | dfv]");

struct alignas(16) MtlLds {
    float lg[3][HB_MAXN];  // logits: fused, audio, visual
    float ex[3][HB_MAXN];
    float dl[2][HB_MAXN];  // what the walks read: g_a (+ g_f), g_v (+ g_f)
    float wmx[3][HB_NW];
    float mx[3], lse[3];
};

// grid = B, a sample per 1024-thread block.  The sample's three loss terms go the way head_cls_ce_kernel's one term goes
// (ticket.h): wave 15 publishes them and draws the ticket, and the block that draws the last one adds the B terms of each loss
// in ticket_fold256's order (= softmax_ce_block's), writes losses[0..2] and hands the counter back at zero.
__global__ __launch_bounds__(1024) void head_mtl_ce_kernel(const float* __restrict__ fa, const float* __restrict__ fv,
                                                          const float* __restrict__ Wa, const float* __restrict__ Wv, int ldw,
                                                          const float* __restrict__ ba, const float* __restrict__ bv, int sum_bias,
                                                          const int64_t* __restrict__ labels, float scale_u, int fused_reaches,
                                                          float* __restrict__ out, float* __restrict__ out_a,
                                                          float* __restrict__ out_v, float* __restrict__ losses,
                                                          float* __restrict__ g_f, float* __restrict__ g_a, float* __restrict__ g_v,
                                                          float* __restrict__ dfa, float* __restrict__ dfv, float* __restrict__ part,
                                                          unsigned* __restrict__ cnt, int B, int n) {
    __shared__ MtlLds s;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        float xa[MTL_ND], xv[MTL_ND];
        head_load_feat<MTL_ND>(fa + (size_t)b * MTL_D, lane, xa);
        head_load_feat<MTL_ND>(fv + (size_t)b * MTL_D, lane, xv);
        for (int j = wave; j < n; j += 2 * HB_NW) {
            const int j2 = j + HB_NW, jr = j2 < n ? j2 : j;
            float pa, pa2, pv, pv2;
            head_dot2<MTL_ND>(Wa + (size_t)j * ldw, Wa + (size_t)jr * ldw, xa, lane, pa, pa2);
            head_dot2<MTL_ND>(Wv + (size_t)j * ldw, Wv + (size_t)jr * ldw, xv, lane, pv, pv2);
            if (lane == 0) {
                const float bx = ba[j], by = bv[j];
                s.lg[0][j] = pa + pv + (sum_bias ? bx + by : bx);
                s.lg[1][j] = pa + bx;
                s.lg[2][j] = pv + by;
                if (j2 < n) {
                    const float bx2 = ba[j2], by2 = bv[j2];
                    s.lg[0][j2] = pa2 + pv2 + (sum_bias ? bx2 + by2 : bx2);
                    s.lg[1][j2] = pa2 + bx2;
                    s.lg[2][j2] = pv2 + by2;
                }
            }
        }
    }
    __syncthreads();
    float* const outs[3] = {out, out_a, out_v};
    float* const gs[3] = {g_f, g_a, g_v};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float m = -INFINITY;
        for (int j = threadIdx.x; j < n; j += 1024) {
            const float l = s.lg[k][j];
            outs[k][(size_t)b * n + j] = l;
            m = fmaxf(m, l);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) s.wmx[k][wave] = m;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float m = s.wmx[k][0];
#pragma unroll
        for (int w = 1; w < HB_NW; ++w) m = fmaxf(m, s.wmx[k][w]);
        if (threadIdx.x == 0) s.mx[k] = m;
        for (int j = threadIdx.x; j < n; j += 1024) s.ex[k][j] = expf(s.lg[k][j] - m);
    }
    __syncthreads();
    if (lane == 0 && wave < 3) {  // the three exp-sums, each in class order, on three waves
        float se = 0.f;
        for (int j = 0; j < n; ++j) se += s.ex[wave][j];
        s.lse[wave] = s.mx[wave] + logf(se);
    }
    __syncthreads();
    const long lab64 = (long)labels[b];
    const int lab = (lab64 >= 0 && lab64 < n) ? (int)lab64 : -1;
    for (int j = threadIdx.x; j < n; j += 1024) {
        const float oh = j == lab ? 1.f : 0.f;
        const float df_ = 1.f * (expf(s.lg[0][j] - s.lse[0]) - oh) / (float)B;
        const float da = scale_u * (expf(s.lg[1][j] - s.lse[1]) - oh) / (float)B;
        const float dv = scale_u * (expf(s.lg[2][j] - s.lse[2]) - oh) / (float)B;
        gs[0][(size_t)b * n + j] = df_;
        gs[1][(size_t)b * n + j] = da;
        gs[2][(size_t)b * n + j] = dv;
        s.dl[0][j] = fused_reaches ? da + df_ : da;
        s.dl[1][j] = fused_reaches ? dv + df_ : dv;
    }
    __syncthreads();  // (the last barrier)
    if (threadIdx.x < MTL_D)
        dfa[(size_t)b * MTL_D + threadIdx.x] = head_df_walk(s.dl[0], Wa, ldw, threadIdx.x, n);
    else
        dfv[(size_t)b * MTL_D + threadIdx.x - MTL_D] = head_df_walk(s.dl[1], Wv, ldw, threadIdx.x - MTL_D, n);
    if (wave == HB_NW - 1) {
        int last = 0;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) st_agent(part + (size_t)k * B + b, lab >= 0 ? s.lse[k] - s.lg[k][lab] : __builtin_nanf(""));
            last = ticket_draw(cnt, B);
        }
        last = __shfl(last, 0);
        if (last) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float t = ticket_fold256(part + (size_t)k * B, B, lane);
                if (lane == 0) losses[k] = t / (float)B;
            }
            if (lane == 0) ticket_hand_back(cnt);
        }
    }
}

// ws: [0] the ticket counter on a 256-byte line of its own, [64 ..) the 3 B loss terms
size_t head_mtl_ce_ws_bytes(int B) { return (64 + 3 * (size_t)(B > 0 ? B : 0)) * sizeof(float); }
int head_mtl_ce(const float* fa, const float* fv, const float* Wa, const float* Wv, int ldw, const float* ba, const float* bv,
                int sum_bias, const int64_t* labels, float scale_u, int fused_reaches, float* out, float* out_a, float* out_v,
                float* losses, float* g_f, float* g_a, float* g_v, float* dfa, float* dfv, int B, int n, void* ws, hipStream_t st) {
    GDL_REQUIRE(n <= HB_MAXN, "head_mtl_ce: at most %d classes", HB_MAXN);
    ProfScope prof("gdl::head_mtl_ce_kernel", PROF_HBM, st, (double)B * MTL_D * 16.0 + (double)n * MTL_D * 8.0 + (double)B * n * 24.0);
    hipLaunchKernelGGL(head_mtl_ce_kernel, dim3(B), dim3(1024), 0, st, fa, fv, Wa, Wv, ldw, ba, bv, sum_bias, labels, scale_u,
                       fused_reaches, out, out_a, out_v, losses, g_f, g_a, g_v, dfa, dfv, (float*)ws + 64, (unsigned*)ws, B, n);
    GDL_CHECK_LAUNCH("head_mtl_ce_kernel");
    return GDL_OK;
}

}  // namespace gdl
