// head_body.h -- one sample's "logits -> cross-entropy gradient -> feature gradient" on a 1024-thread block, and the dot and
// walk helpers it is made of.  head_uni_dfeat_kernel (head.hip, the DGL step) IS this body; head_cls_ce_kernel (head_cls.hip,
// the unimodal step) is this body with its two stores compiled in (STORE), plus the sample's loss term and the loss sum;
// head_cls_fwd_kernel / head_cls_dfeat_kernel use the helpers; linprobe_ce_kernel (linprobe.hip, the linear probe's fit) is the
// body's first part, head_ce_logits, on a row gathered from a feature bank.  Every sum has ONE order and ONE spelling -- an explicit
// fmaf chain, here and in the kernels of head.hip / head_film.hip whose orders these reproduce:
//   a logit      : lane l of a wave adds W[j][l + 64 i] * f[l + 64 i] for i = 0 .. ND-1 (fmaf chain), xor butterfly 32 .. 1, + b[j]
//   softmax / CE : softmax_ce_block's (head.hip) -- max (exact in any order), expf(l - max) summed in class order,
//                  lse = max + logf(sum), dlogits = scale * (expf(l - lse) - onehot) / B
//   df[i]        : classes in ascending order (fmaf chain), eight weight loads in flight
// which is the order of head_fwd_kernel + softmax_ce_block + head_bwd_feat_kernel and of head_cls_fwd + softmax_ce +
// head_cls_bwd: df (and head_cls_ce's out and dlogits) carry the bits of those three-launch paths.
#pragma once
#include "common.h"

namespace gdl {

constexpr int HB_MAXN = 512;  // classes the body stages in LDS
constexpr int HB_NW = 16;     // waves of the body's block

template <int ND>  // feature width = 64 ND
__device__ __forceinline__ void head_load_feat(const float* __restrict__ f, int lane, float (&fv)[ND]) {
#pragma unroll
    for (int i = 0; i < ND; ++i) fv[i] = f[lane + 64 * i];
}
// the lane's share of two logits at a time (their loads and butterflies overlap); every lane returns the full sums
template <int ND>
__device__ __forceinline__ void head_dot2(const float* __restrict__ w, const float* __restrict__ w2, const float (&fv)[ND], int lane,
                                          float& pa, float& pb) {
    pa = 0.f, pb = 0.f;
#pragma unroll
    for (int i = 0; i < ND; ++i) pa = fmaf(w[lane + 64 * i], fv[i], pa);
#pragma unroll
    for (int i = 0; i < ND; ++i) pb = fmaf(w2[lane + 64 * i], fv[i], pb);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pa += __shfl_xor(pa, o);
        pb += __shfl_xor(pb, o);
    }
}
// df[i] = sum_j g[j] W[j][i] (row pitch ldw), classes ascending; g in LDS
__device__ __forceinline__ float head_df_walk(const float* g, const float* __restrict__ W, int ldw, int i, int n) {
    const float* w = W + i;
    float s = 0.f;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = w[(size_t)(j + u) * ldw];
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(g[j + u], q[u], s);
    }
    for (; j < n; ++j) s = fmaf(g[j], w[(size_t)j * ldw], s);
    return s;
}

// what the body leaves in LDS for its caller: the sample's logits, their gradient, logsumexp (16-byte aligned: the walks
// over dl and ex read four floats per ds_read_b128)
struct alignas(16) HeadBodyLds {
    float lg[HB_MAXN], dl[HB_MAXN], ex[HB_MAXN];
    float wmx[HB_NW];
    float lse;
};

// One sample's logits, softmax and logit gradient on a 1024-thread block, up to and including the last barrier: fb the sample's
// features, lab_p its label, out_b / dl_b its rows of out[B, n] / dlogits[B, n] (STORE only); B the divisor of the mean.  16 waves
// per sample and no serial walk beyond the sums whose order is the contract: the classes go round the 16 waves two at a time,
// max and exp are evaluated by all threads (max is exact in any order; the exponentials are the same values) and only their SUM
// is walked in class order by one thread.  Leaves s.lg, s.dl and s.lse for the caller.  head_ce_body below is this plus the
// feature gradient; linprobe_ce_kernel (linprobe.hip) is this on a gathered row.
// STORE: the logits and their gradient also go to out_b / dl_b, from the loops that have them in a register (the max and the dl
// loop); without it the two pointers are not read.
// Returns the sample's label, -1 for a class index outside [0, n) (a device assert in the reference's CrossEntropyLoss): no
// one-hot term then.
template <int ND, bool STORE>
__device__ __forceinline__ int head_ce_logits(HeadBodyLds& s, const float* __restrict__ fb, const float* __restrict__ W, int ldw,
                                              const float* __restrict__ bias, const int64_t* __restrict__ lab_p, float scale,
                                              float* __restrict__ out_b, float* __restrict__ dl_b, int B, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float fv[ND];
    head_load_feat<ND>(fb, lane, fv);
    for (int j = wave; j < n; j += 2 * HB_NW) {
        const int j2 = j + HB_NW;
        float pa, pb;
        head_dot2<ND>(W + (size_t)j * ldw, W + (size_t)(j2 < n ? j2 : j) * ldw, fv, lane, pa, pb);
        if (lane == 0) {
            s.lg[j] = pa + bias[j];
            if (j2 < n) s.lg[j2] = pb + bias[j2];
        }
    }
    __syncthreads();
    {
        float mx = -INFINITY;
        for (int j = threadIdx.x; j < n; j += 1024) {
            const float l = s.lg[j];
            if (STORE) out_b[j] = l;
            mx = fmaxf(mx, l);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) s.wmx[wave] = mx;
    }
    __syncthreads();
    float mx = s.wmx[0];
#pragma unroll
    for (int w = 1; w < HB_NW; ++w) mx = fmaxf(mx, s.wmx[w]);
    for (int j = threadIdx.x; j < n; j += 1024) s.ex[j] = expf(s.lg[j] - mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        float se = 0.f;
        for (int j = 0; j < n; ++j) se += s.ex[j];
        s.lse = mx + logf(se);
    }
    __syncthreads();
    const long lab64 = (long)lab_p[0];
    const int lab = (lab64 >= 0 && lab64 < n) ? (int)lab64 : -1;
    const float lse = s.lse;
    for (int j = threadIdx.x; j < n; j += 1024) {
        const float d = scale * (expf(s.lg[j] - lse) - (j == lab ? 1.f : 0.f)) / (float)B;
        s.dl[j] = d;
        if (STORE) dl_b[j] = d;
    }
    __syncthreads();  // (the last barrier: from here on the waves part ways)
    return lab;
}

// Sample b = blockIdx.x of a grid of B blocks of 1024 threads; n <= HB_MAXN: head_ce_logits on row b, then df[b], written by the
// threads < 64 ND in strides of 1024, so behind the last barrier the other waves are free.  STORE and the return value: as above.
template <int ND, bool STORE>
__device__ __forceinline__ int head_ce_body(HeadBodyLds& s, const float* __restrict__ f, const float* __restrict__ W, int ldw,
                                            const float* __restrict__ bias, const int64_t* __restrict__ labels, float scale,
                                            float* __restrict__ out, float* __restrict__ dlogits, float* __restrict__ df, int B,
                                            int n) {
    constexpr int D = 64 * ND;
    const int b = blockIdx.x;
    const int lab = head_ce_logits<ND, STORE>(s, f + (size_t)b * D, W, ldw, bias, labels + b, scale,
                                              STORE ? out + (size_t)b * n : nullptr, STORE ? dlogits + (size_t)b * n : nullptr, B, n);
    for (int i = threadIdx.x; i < D; i += 1024) df[(size_t)b * D + i] = head_df_walk(s.dl, W, ldw, i, n);
    return lab;
}

}  // namespace gdl
