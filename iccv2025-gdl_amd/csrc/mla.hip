// mla.hip -- alternating unimodal training with a shared head (MLA, Zhang et al., CVPR 2024): the projector that shapes the
// shared head's weight gradient, and the entropy-weighted test-time fusion of the two unimodal logit sets.  All float32, no
// floating-point atomic, no block ever waits for another, every sum in ONE order that does not depend on the launch geometry:
// two runs give identical bytes.  DESIGN.md section 8 states the arithmetic; tests/mla_ref.py restates it in float64.
//
// The one dot product of this file, dot512(x, y): lane l of a wave adds x[l + 64 m] y[l + 64 m] for m = 0 .. 7 as one fmaf chain
// from 0, then the xor butterfly 32 .. 1 (every lane ends with the same sum).
//
//   mla_feature_mean   r[k] = (sum_b h[b][k]) / B: a thread per feature, plain adds with b ascending from 0, one division.
//   mla_projector_update, the recursive update of P [512][512] against r [512], two launches or three (no block waits for
//                      another, and a block that recomputed k = P r itself would read rows that other blocks are rewriting):
//     1. k[i] = dot512(P[i], r)                                    grid 128 x 256, a wave per row; k goes to the workspace
//     2. c = alpha + dot512(r, k) by every wave (all hold the same bits);  P[i][j] = P[i][j] - (k[i] k[j]) / c: the product
//        rounded, one division, one subtraction, none of them contracted -- k[i] k[j] = k[j] k[i] in floating point, so a
//        symmetric P stays symmetric bit for bit.  normalize: rowsq[i] = the squares of the NEW row as dot512(P[i], P[i]).
//     3. (normalize)  S = the 512 row sums in double: lane l adds rowsq[l + 64 m], m ascending, then the xor butterfly -- by
//        every wave; P[i][j] = P[i][j] / (float)sqrt(S), one division.
//   mla_project        dW [n][512] <- dW P^T in place: out[c][i] = dot512(dW[c], P[i]).  A block owns R = 1 (n <= 64) or 4 whole
//                      rows of dW: every wave loads them into registers, ONE barrier, then wave w computes i = 64 w .. 64 w + 63
//                      and lane t keeps i = 64 w + t, so the store is one coalesced line per row.  The sum's order is dot512's
//                      whatever R is.
//   mla_fuse           a block per sample, a wave per modality: lse = max + logf(sum_j expf(l_j - max)) (head_body.h's spelling:
//                      the exponentials staged in LDS and added in ascending class order by one lane), p_j = expf(l_j - lse),
//                      e = sum_j p_j (lse - l_j) in ascending class order (lse >= max: the maximum's own exponential is exactly 1,
//                      so every term is >= 0; a p_j that underflows to 0 contributes 0), w_m = expf(-(e_m - min(e_a, e_v))),
//                      lam_m = w_m / (w_a + w_v), out = lam_a out_a + lam_v out_v (two rounded products, one add).  Equal
//                      entropies give w = 1, 1 and lam = 0.5 exactly.  A NaN or inf logit makes its row's lse NaN, hence both lam
//                      and the whole out row NaN.  dynamic = 0: lam = 0.5, 0.5 and nothing else is computed.
#include "common.h"
#include "head_body.h"
#include "ops.h"

// The products, sums and differences spelled below are the arithmetic: nothing in this file is contracted into a fused
// multiply-add behind the source's back (the chains that ARE fused say fmaf).
#pragma clang fp contract(off)

namespace gdl {

constexpr int ML_D = 512;          // feature width = the projector's side
constexpr int ML_ND = ML_D / 64;   // elements per lane of a row
constexpr int ML_RW = 4;           // rows (waves) per block of the projector launches

__device__ __forceinline__ float mla_butterfly(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__device__ __forceinline__ float mla_dot512(const float* __restrict__ x, const float* __restrict__ y, int lane) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < ML_ND; ++m) s = fmaf(x[lane + 64 * m], y[lane + 64 * m], s);
    return mla_butterfly(s);
}

__global__ __launch_bounds__(256) void mla_feature_mean_kernel(const float* __restrict__ h, int B, float* __restrict__ r) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const float* __restrict__ p = h + k;
    float s = 0.f;
    int b = 0;
    for (; b + 4 <= B; b += 4) {  // four rows in flight, added in row order
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p[(size_t)(b + e) * ML_D];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = __fadd_rn(s, v[e]);
    }
    for (; b < B; ++b) s = __fadd_rn(s, p[(size_t)b * ML_D]);
    r[k] = __fdiv_rn(s, (float)B);
}

__global__ __launch_bounds__(64 * ML_RW) void mla_k_kernel(const float* __restrict__ P, const float* __restrict__ r,
                                                          float* __restrict__ k) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * ML_RW + (threadIdx.x >> 6);
    const float s = mla_dot512(P + (size_t)i * ML_D, r, lane);
    if (lane == 0) k[i] = s;
}

__global__ __launch_bounds__(64 * ML_RW) void mla_rank1_kernel(float* __restrict__ P, const float* __restrict__ r,
                                                              const float* __restrict__ k, float alpha,
                                                              float* __restrict__ rowsq) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * ML_RW + (threadIdx.x >> 6);
    const float c = __fadd_rn(alpha, mla_dot512(r, k, lane));
    const float ki = k[i];
    float* __restrict__ row = P + (size_t)i * ML_D;
    float sq = 0.f;
#pragma unroll
    for (int m = 0; m < ML_ND; ++m) {
        const int j = lane + 64 * m;
        const float v = __fsub_rn(row[j], __fdiv_rn(__fmul_rn(ki, k[j]), c));
        row[j] = v;
        sq = fmaf(v, v, sq);
    }
    if (rowsq) {
        sq = mla_butterfly(sq);
        if (lane == 0) rowsq[i] = sq;
    }
}

__global__ __launch_bounds__(64 * ML_RW) void mla_normalize_kernel(float* __restrict__ P, const float* __restrict__ rowsq) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * ML_RW + (threadIdx.x >> 6);
    double S = 0.0;
#pragma unroll
    for (int m = 0; m < ML_ND; ++m) S += (double)rowsq[lane + 64 * m];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    const float nrm = (float)sqrt(S);
    float* __restrict__ row = P + (size_t)i * ML_D;
#pragma unroll
    for (int m = 0; m < ML_ND; ++m) row[lane + 64 * m] = __fdiv_rn(row[lane + 64 * m], nrm);
}

template <int R>
__global__ __launch_bounds__(512) void mla_project_kernel(float* __restrict__ dW, const float* __restrict__ P, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = blockIdx.x * R;
    float dv[R][ML_ND];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const bool live = c0 + q < n;
#pragma unroll
        for (int m = 0; m < ML_ND; ++m) dv[q][m] = live ? dW[(size_t)(c0 + q) * ML_D + lane + 64 * m] : 0.f;
    }
    __syncthreads();  // every wave holds the block's rows: from here on they may be overwritten
    float keep[R];
#pragma unroll
    for (int q = 0; q < R; ++q) keep[q] = 0.f;
#pragma unroll 2
    for (int t = 0; t < 64; ++t) {
        const float* __restrict__ prow = P + (size_t)(wave * 64 + t) * ML_D;
        float pv[ML_ND];
#pragma unroll
        for (int m = 0; m < ML_ND; ++m) pv[m] = prow[lane + 64 * m];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < ML_ND; ++m) s = fmaf(dv[q][m], pv[m], s);
            s = mla_butterfly(s);
            if (lane == t) keep[q] = s;
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q)
        if (c0 + q < n) dW[(size_t)(c0 + q) * ML_D + wave * 64 + lane] = keep[q];
}

__global__ __launch_bounds__(128) void mla_fuse_kernel(const float* __restrict__ out_a, const float* __restrict__ out_v, int n,
                                                      int dynamic, float* __restrict__ out, float* __restrict__ lam) {
    __shared__ float tm[2][HB_MAXN];
    __shared__ float ent[2];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ ra = out_a + (size_t)b * n;
    const float* __restrict__ rv = out_v + (size_t)b * n;
    float la = 0.5f, lv = 0.5f;
    if (dynamic) {
        const float* __restrict__ l = wave == 0 ? ra : rv;
        float mx = -INFINITY;
        for (int j = lane; j < n; j += 64) mx = fmaxf(mx, l[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        for (int j = lane; j < n; j += 64) tm[wave][j] = expf(l[j] - mx);
        __syncthreads();
        float lse = 0.f;
        if (lane == 0) {
            float se = 0.f;
            for (int j = 0; j < n; ++j) se += tm[wave][j];
            lse = mx + logf(se);
        }
        lse = __shfl(lse, 0);
        __syncthreads();  // (the exponentials are read: their slots take the entropy terms)
        for (int j = lane; j < n; j += 64) {
            const float lj = l[j];
            tm[wave][j] = __fmul_rn(expf(lj - lse), lse - lj);
        }
        __syncthreads();
        if (lane == 0) {
            float e = 0.f;
            for (int j = 0; j < n; ++j) e = __fadd_rn(e, tm[wave][j]);
            ent[wave] = e;
        }
        __syncthreads();
        const float ea = ent[0], ev = ent[1], mn = fminf(ea, ev);
        const float wa = expf(-__fsub_rn(ea, mn)), wv = expf(-__fsub_rn(ev, mn));
        const float den = __fadd_rn(wa, wv);
        la = __fdiv_rn(wa, den), lv = __fdiv_rn(wv, den);
    }
    for (int j = threadIdx.x; j < n; j += 128) out[(size_t)b * n + j] = __fadd_rn(__fmul_rn(la, ra[j]), __fmul_rn(lv, rv[j]));
    if (lam && threadIdx.x == 0) lam[2 * b] = la, lam[2 * b + 1] = lv;
}

int mla_feature_mean(const float* h, int B, float* r, hipStream_t st) {
    hipLaunchKernelGGL(mla_feature_mean_kernel, dim3(ML_D / 256), dim3(256), 0, st, h, B, r);
    GDL_CHECK_LAUNCH("mla_feature_mean_kernel");
    return GDL_OK;
}

size_t mla_projector_ws_bytes() { return 2 * ML_D * sizeof(float); }  // k [512] | rowsq [512]

int mla_projector_update(float* P, const float* r, float alpha, int normalize, void* ws, hipStream_t st) {
    float* k = (float*)ws;
    float* rowsq = k + ML_D;
    hipLaunchKernelGGL(mla_k_kernel, dim3(ML_D / ML_RW), dim3(64 * ML_RW), 0, st, P, r, k);
    GDL_CHECK_LAUNCH("mla_k_kernel");
    hipLaunchKernelGGL(mla_rank1_kernel, dim3(ML_D / ML_RW), dim3(64 * ML_RW), 0, st, P, r, k, alpha, normalize ? rowsq : nullptr);
    GDL_CHECK_LAUNCH("mla_rank1_kernel");
    if (normalize) {
        hipLaunchKernelGGL(mla_normalize_kernel, dim3(ML_D / ML_RW), dim3(64 * ML_RW), 0, st, P, rowsq);
        GDL_CHECK_LAUNCH("mla_normalize_kernel");
    }
    return GDL_OK;
}

int mla_project(float* dW, const float* P, int n, hipStream_t st) {
    if (n <= 64)
        hipLaunchKernelGGL(mla_project_kernel<1>, dim3(n), dim3(512), 0, st, dW, P, n);
    else
        hipLaunchKernelGGL(mla_project_kernel<4>, dim3(ceil_div(n, 4)), dim3(512), 0, st, dW, P, n);
    GDL_CHECK_LAUNCH("mla_project_kernel");
    return GDL_OK;
}

int mla_fuse(const float* out_a, const float* out_v, int B, int n, int dynamic, float* out, float* lam, hipStream_t st) {
    hipLaunchKernelGGL(mla_fuse_kernel, dim3(B), dim3(128), 0, st, out_a, out_v, n, dynamic, out, lam);
    GDL_CHECK_LAUNCH("mla_fuse_kernel");
    return GDL_OK;
}

}  // namespace gdl
