// pareto.hip -- MMPareto gradient integration (Wei & Hu, ICML 2024; DESIGN.md section 8 is this project's statement of the
// arithmetic, tests/pareto_ref.py restates it in float64): one encoder's gradient of the fused loss, g_m, and of its own unimodal
// loss, g_u, both n float32 in arenas that are only 4-byte aligned, become ONE gradient written over g_m.  Two launches, no
// floating-point atomic, no block waits for another, every sum in ONE order that depends on n alone -- not on the grid, the stream
// or the alignment of either pointer: two calls on the same values give the same bytes wherever the vectors lie.
//
//   1. pareto_dots_kernel      block c owns the elements [8192 c, 8192 (c + 1)).  Thread t takes the groups of four elements
//                              4 (t + 256 k) .. + 3, k = 0 .. 7, and adds g_m^2, g_u^2 and g_m g_u -- each product formed in double,
//                              where it is exact -- to three double sums, k ascending and the four elements of a group in turn;
//                              the 256 sums are folded by the tree p[i] += p[i + o], o = 128 .. 1, and p[0] goes to
//                              partial[q][c].  The groups are addressed by their element index, so a thread sees the same elements
//                              whatever the pointers' alignment: its loads are 16 bytes wide at 4-byte alignment (a multi-dword
//                              global access needs dword alignment only), the last block of an n that is no multiple of 8192
//                              loads element by element under a bound check, in the same order.
//   2. pareto_combine_kernel   every block folds partial[q][0 .. chunks) itself, in the same order -- thread t adds partials
//                              t, t + 256, .., then the same tree -- and computes, in double, none of it contracted:
//                                S_mu > 0 and all three sums finite (agreement):  D = S_mm - 2 S_mu + S_uu,
//                                    gamma = D > 0 ? clamp((S_uu - S_mu) / D, 0, 1) : 0.5,  w_m = 2 gamma,  w_u = 2 (1 - gamma)
//                                otherwise (sum):  gamma = 0.5,  w_m = w_u = 1
//                                N_h^2 = w_m^2 S_mm + 2 w_m w_u S_mu + w_u^2 S_uu,   N_s^2 = S_mm + 2 S_mu + S_uu
//                                s = agreement and N_h^2 > 0 and finite ? sqrt(N_s^2 / N_h^2) : 1
//                                c_m = (float)(scale s w_m),  c_u = (float)(scale s w_u)
//                              then over its own 8192 elements  g_m[i] = fmaf(c_u, g_u[i], c_m * g_m[i])  (the product rounded).
//                              g_m is loaded and stored 16 bytes wide over the 16-byte aligned middle of the block's range, with
//                              up to three elements peeled in front and behind; g_u is read 16 bytes wide at 4-byte alignment.
//                              Block 0 writes info[8] = {S_mm, S_uu, S_mu, gamma, w_m, w_u, s, agreement ? 1 : 0} and leaves
//                              {c_m, c_u} in the first two floats of the workspace.
#include "common.h"
#include "ops.h"

// The products, sums and differences spelled below are the arithmetic: nothing in this file is contracted into a fused
// multiply-add behind the source's back (the one that IS fused says fmaf).
#pragma clang fp contract(off)

namespace gdl {

constexpr int PR_CHUNK = 8192;  // elements per block of both launches: 8 groups of four per thread, 16 loads of 16 bytes in flight
constexpr int PR_NT = 256;
constexpr int PR_NK = PR_CHUNK / (4 * PR_NT);
constexpr size_t PR_HEAD = 16;  // bytes in front of the partials: {c_m, c_u, 0, 0}

typedef float pr_f4u __attribute__((ext_vector_type(4), aligned(4)));  // four floats behind a pointer that is 4-byte aligned

static inline int64_t pareto_chunks(int64_t n) { return (n + PR_CHUNK - 1) / PR_CHUNK; }

// p[0] = the sum of p[0 .. 256) by the tree o = 128 .. 1, for each of the three rows (all threads of the block call it)
__device__ __forceinline__ void pareto_tree(double (*sh)[PR_NT]) {
    __syncthreads();
    for (int o = PR_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + o];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PR_NT) void pareto_dots_kernel(const float* __restrict__ gm, const float* __restrict__ gu, int64_t n,
                                                           int64_t chunks, double* __restrict__ partial) {
    __shared__ double sh[3][PR_NT];
    const int64_t c0 = (int64_t)blockIdx.x * PR_CHUNK;
    const int t = threadIdx.x;
    double mm = 0.0, uu = 0.0, mu = 0.0;
    if (c0 + PR_CHUNK <= n) {
        pr_f4u a[PR_NK], b[PR_NK];
#pragma unroll
        for (int k = 0; k < PR_NK; ++k) {
            a[k] = *(const pr_f4u*)(gm + c0 + 4 * (t + PR_NT * k));
            b[k] = *(const pr_f4u*)(gu + c0 + 4 * (t + PR_NT * k));
        }
#pragma unroll
        for (int k = 0; k < PR_NK; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double x = (double)a[k][e], y = (double)b[k][e];
                mm += x * x;
                uu += y * y;
                mu += x * y;
            }
    } else {
        for (int k = 0; k < PR_NK; ++k)
            for (int e = 0; e < 4; ++e) {
                const int64_t i = c0 + 4 * (t + PR_NT * k) + e;
                if (i < n) {
                    const double x = (double)gm[i], y = (double)gu[i];
                    mm += x * x;
                    uu += y * y;
                    mu += x * y;
                }
            }
    }
    sh[0][t] = mm, sh[1][t] = uu, sh[2][t] = mu;
    pareto_tree(sh);
    if (t < 3) partial[(size_t)t * chunks + blockIdx.x] = sh[t][0];
}

__global__ __launch_bounds__(PR_NT) void pareto_combine_kernel(float* __restrict__ gm, const float* __restrict__ gu, int64_t n,
                                                              int64_t chunks, const double* __restrict__ partial, float scale,
                                                              float* __restrict__ info, float* __restrict__ coef) {
    __shared__ double sh[3][PR_NT];
    const int t = threadIdx.x;
    {
        double a[3] = {0.0, 0.0, 0.0};
        for (int64_t c = t; c < chunks; c += PR_NT)
#pragma unroll
            for (int q = 0; q < 3; ++q) a[q] += partial[(size_t)q * chunks + c];
#pragma unroll
        for (int q = 0; q < 3; ++q) sh[q][t] = a[q];
    }
    pareto_tree(sh);
    const double Smm = sh[0][0], Suu = sh[1][0], Smu = sh[2][0];
    const bool fin = isfinite(Smm) && isfinite(Suu) && isfinite(Smu);
    const bool agree = fin && Smu > 0.0;
    double gamma = 0.5, wm = 1.0, wu = 1.0, s = 1.0;
    if (agree) {
        const double D = Smm - 2.0 * Smu + Suu;
        if (D > 0.0) gamma = fmin(fmax((Suu - Smu) / D, 0.0), 1.0);
        wm = 2.0 * gamma;
        wu = 2.0 * (1.0 - gamma);
        const double Nh2 = wm * wm * Smm + 2.0 * wm * wu * Smu + wu * wu * Suu;
        const double Ns2 = Smm + 2.0 * Smu + Suu;
        if (Nh2 > 0.0 && isfinite(Nh2)) s = sqrt(Ns2 / Nh2);
    }
    const float cm = (float)((double)scale * s * wm), cu = (float)((double)scale * s * wu);
    if (blockIdx.x == 0 && t == 0) {
        info[0] = (float)Smm, info[1] = (float)Suu, info[2] = (float)Smu, info[3] = (float)gamma;
        info[4] = (float)wm, info[5] = (float)wu, info[6] = (float)s, info[7] = agree ? 1.f : 0.f;
        coef[0] = cm, coef[1] = cu;
    }
    // the block's range: scalar ends around the 16-byte aligned middle of g_m
    const int64_t c0 = (int64_t)blockIdx.x * PR_CHUNK;
    const int len = (int)((n - c0) < PR_CHUNK ? (n - c0) : PR_CHUNK);
    float* __restrict__ p = gm + c0;
    const float* __restrict__ q = gu + c0;
    const int head = min(len, (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    const int nv = (len - head) >> 2;
    for (int i = t; i < nv; i += PR_NT) {
        float4 v = *(float4*)(p + head + 4 * i);
        const pr_f4u w = *(const pr_f4u*)(q + head + 4 * i);
        v.x = fmaf(cu, w[0], __fmul_rn(cm, v.x));
        v.y = fmaf(cu, w[1], __fmul_rn(cm, v.y));
        v.z = fmaf(cu, w[2], __fmul_rn(cm, v.z));
        v.w = fmaf(cu, w[3], __fmul_rn(cm, v.w));
        *(float4*)(p + head + 4 * i) = v;
    }
    {  // at most 3 elements in front of and 3 behind the aligned middle: threads 0 .. head - 1 and head .. head + tail - 1
        const int tail = len - head - 4 * nv;
        const int i = t < head ? t : head + 4 * nv + (t - head);
        if (t < head + tail) p[i] = fmaf(cu, q[i], __fmul_rn(cm, p[i]));
    }
}

size_t pareto_ws_bytes(int64_t n) { return n > 0 ? PR_HEAD + (size_t)pareto_chunks(n) * 3 * sizeof(double) : 0; }

int pareto_integrate(float* g_m, const float* g_u, int64_t n, float scale, float* info, void* ws, hipStream_t st) {
    const int64_t chunks = pareto_chunks(n);
    float* coef = (float*)ws;
    double* partial = (double*)((char*)ws + PR_HEAD);
    hipLaunchKernelGGL(pareto_dots_kernel, dim3((unsigned)chunks), dim3(PR_NT), 0, st, (const float*)g_m, g_u, n, chunks, partial);
    GDL_CHECK_LAUNCH("pareto_dots_kernel");
    hipLaunchKernelGGL(pareto_combine_kernel, dim3((unsigned)chunks), dim3(PR_NT), 0, st, g_m, g_u, n, chunks,
                       (const double*)partial, scale, info, coef);
    GDL_CHECK_LAUNCH("pareto_combine_kernel");
    return GDL_OK;
}

}  // namespace gdl
