// proto.hip -- prototypical modal rebalance (PMR, Fan et al., CVPR 2023) on the joint step: a prototype cross-entropy on each
// encoder's pooled 512-wide feature, added to the joint loss for whichever modality is behind.  All float32, no floating-point
// atomic, no block ever waits for another, every sum in ONE order: two runs give identical bytes.  DESIGN.md section 8 states
// the arithmetic; tests/pmr_ref.py restates it in float64.
//
// For a modality with features f [B][512], class prototypes P [n][512] (n <= 512) and labels [B]:
//   d[b][j] = sqrt(sum_k (f[b][k] - P[j][k])^2),  sim = -d,  p = softmax(sim),  score = sum_b p[b][label_b],
//   lossp = (1/B) sum_b (lse_b - sim[b][label_b]),  u[b][k] = d lossp / d f[b][k] = sum_j q[b][j] (P[j][k] - f[b][k]),
//   q[b][j] = ((p[b][j] - [j == label_b]) / B) / d[b][j]   (0 where d = 0: torch's sqrt backward gives NaN there)
// Three launchers:
//   proto_ce      one launch per modality, grid B x 1024 (head_body.h's geometry: the classes go round the 16 waves two at a
//                 time, eight features per lane).  The squared distance is the direct sum of squared differences -- lane l adds
//                 (f[l + 64 i] - P[j][l + 64 i])^2 for i = 0 .. 7 as one fmaf chain, then the xor butterfly 32 .. 1 -- never the
//                 |f|^2 - 2 f.P + |P|^2 expansion, which cancels; ONE sqrtf; the softmax in head_ce_logits' spelling (row max,
//                 expf, the exponentials summed in ascending class order by one thread, lse = max + logf(sum), p = expf(sim - lse));
//                 q staged in LDS; then one thread per feature walks the classes in ascending order as one fmaf chain
//                 (head_df_walk's shape, eight prototype loads in flight, coalesced across k).  Writes u [B][512], the sample's
//                 two terms (terms[b] = p[b][label], terms[B + b] = lse_b - sim[b][label]) and, if asked, sim [B][n].  A label
//                 outside [0, n): no one-hot term, a score term of 0, a NaN loss term (the head kernels' convention).
//   proto_apply   one launch, grid ceil(B 128 / 256) x 256: EVERY block folds the 4 B terms itself in ticket_fold256's order (one
//                 wave per term array; the terms come from earlier launches the stream has ordered, so there is no ticket and no
//                 counter), hence all blocks hold the same score_a, score_v, rho = score_a / score_v and
//                   rho > 1: beta = 0, lam = alpha;   rho < 1: beta = alpha, lam = 0;   else (rho == 1 or NaN): beta = lam = 0
//                 then dfa = fmaf(beta, u_a, dfa), dfv = fmaf(lam, u_v, dfv) on its own 256 float4 -- a side whose coefficient is
//                 0 is neither read nor written.  Block 0 writes stats[8] = {score_a, score_v, rho, beta, lam, lossp_a, lossp_v, 0}.
//   proto_update  one launch per feature bank, grid n x 512: block c walks the WHOLE bank in ascending row order (the sample
//                 range is not split: there are no partial sums to combine), a thread per feature adding the rows of class c into a
//                 float64 accumulator; mean = sum / count, P_c = mean (first update) or (1 - momentum) P_c + momentum mean in
//                 float64, rounded to float32 once.  A class without a row keeps its prototype.  count[c] by block c; block 0 also
//                 writes info = {classes without a row, rows whose label is outside [0, n) (they belong to no class)}.
#include "common.h"
#include "head_body.h"
#include "ops.h"
#include "ticket.h"

namespace gdl {

constexpr int PR_D = 512;  // feature width
constexpr int PR_ND = 8;   // features per lane

// two squared distances at a time (their loads and butterflies overlap); every lane returns the full sums
__device__ __forceinline__ void proto_dist2(const float* __restrict__ p, const float* __restrict__ p2, const float (&fv)[PR_ND], int lane,
                                            float& da, float& db) {
    da = 0.f, db = 0.f;
#pragma unroll
    for (int i = 0; i < PR_ND; ++i) {
        const float t = fv[i] - p[lane + 64 * i];
        da = fmaf(t, t, da);
    }
#pragma unroll
    for (int i = 0; i < PR_ND; ++i) {
        const float t = fv[i] - p2[lane + 64 * i];
        db = fmaf(t, t, db);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        da += __shfl_xor(da, o);
        db += __shfl_xor(db, o);
    }
}

// u[k] = sum_j q[j] (P[j][k] - fk), classes ascending, one fmaf chain; q in LDS
__device__ __forceinline__ float proto_u_walk(const float* q, const float* __restrict__ P, float fk, int k, int n) {
    const float* p = P + k;
    float s = 0.f;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = p[(size_t)(j + e) * PR_D];
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(q[j + e], r[e] - fk, s);
    }
    for (; j < n; ++j) s = fmaf(q[j], p[(size_t)j * PR_D] - fk, s);
    return s;
}

// s.lg = sim, s.ex = the exponentials, s.dl = q.  The max / exp / sum / lse lines are head_ce_logits' (head_body.h), restated here
// rather than shared: that function's loops also take the bias, store the logits and form the logit gradient in the same passes.
__global__ __launch_bounds__(1024) void proto_ce_kernel(const float* __restrict__ f, const float* __restrict__ P,
                                                       const int64_t* __restrict__ labels, float* __restrict__ u,
                                                       float* __restrict__ terms, float* __restrict__ sim, int B, int n) {
    __shared__ HeadBodyLds s;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ fb = f + (size_t)b * PR_D;
    float fv[PR_ND];
    head_load_feat<PR_ND>(fb, lane, fv);
    for (int j = wave; j < n; j += 2 * HB_NW) {
        const int j2 = j + HB_NW;
        float da, db;
        proto_dist2(P + (size_t)j * PR_D, P + (size_t)(j2 < n ? j2 : j) * PR_D, fv, lane, da, db);
        if (lane == 0) {
            s.lg[j] = -sqrtf(da);
            if (j2 < n) s.lg[j2] = -sqrtf(db);
        }
    }
    __syncthreads();
    {
        float mx = -INFINITY;
        for (int j = threadIdx.x; j < n; j += 1024) {
            const float l = s.lg[j];
            if (sim) sim[(size_t)b * n + j] = l;
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
    const long lab64 = (long)labels[b];
    const int lab = (lab64 >= 0 && lab64 < n) ? (int)lab64 : -1;
    const float lse = s.lse;
    for (int j = threadIdx.x; j < n; j += 1024) {
        const float l = s.lg[j], d = -l;
        const float g = (expf(l - lse) - (j == lab ? 1.f : 0.f)) / (float)B;
        s.dl[j] = d == 0.f ? 0.f : g / d;  // (a feature row ON a prototype: no gradient from that class; a NaN distance stays NaN)
    }
    if (threadIdx.x == 0) {
        terms[b] = lab >= 0 ? expf(s.lg[lab] - lse) : 0.f;
        terms[B + b] = lab >= 0 ? lse - s.lg[lab] : __builtin_nanf("");
    }
    __syncthreads();  // (the last barrier: the waves beyond the 512 features are done)
    for (int k = threadIdx.x; k < PR_D; k += 1024) u[(size_t)b * PR_D + k] = proto_u_walk(s.dl, P, fb[k], k, n);
}

constexpr int PA_NT = 256;

__global__ __launch_bounds__(PA_NT) void proto_apply_kernel(const float* __restrict__ terms_a, const float* __restrict__ terms_v,
                                                           const float4* __restrict__ u_a, const float4* __restrict__ u_v,
                                                           float4* __restrict__ dfa, float4* __restrict__ dfv, float alpha,
                                                           float* __restrict__ stats, int B) {
    __shared__ float sum[4];  // score_a, the audio loss terms' sum, score_v, the visual loss terms' sum
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    {
        const float v = ticket_fold256((wave < 2 ? terms_a : terms_v) + (wave & 1) * B, B, lane);
        if (lane == 0) sum[wave] = v;
    }
    __syncthreads();
    const float sa = sum[0], sv = sum[2];
    const float rho = sa / sv;
    const float beta = rho < 1.f ? alpha : 0.f, lam = rho > 1.f ? alpha : 0.f;  // (rho == 1, or NaN: neither)
    if (blockIdx.x == 0 && t == 0) {
        stats[0] = sa, stats[1] = sv, stats[2] = rho, stats[3] = beta, stats[4] = lam;
        stats[5] = sum[1] / (float)B, stats[6] = sum[3] / (float)B, stats[7] = 0.f;
    }
    const int q = blockIdx.x * PA_NT + t;
    if (q >= B * (PR_D / 4)) return;
    if (beta != 0.f) {
        const float4 x = u_a[q];
        float4 g = dfa[q];
        g.x = fmaf(beta, x.x, g.x), g.y = fmaf(beta, x.y, g.y), g.z = fmaf(beta, x.z, g.z), g.w = fmaf(beta, x.w, g.w);
        dfa[q] = g;
    }
    if (lam != 0.f) {
        const float4 x = u_v[q];
        float4 g = dfv[q];
        g.x = fmaf(lam, x.x, g.x), g.y = fmaf(lam, x.y, g.y), g.z = fmaf(lam, x.z, g.z), g.w = fmaf(lam, x.w, g.w);
        dfv[q] = g;
    }
}
static_assert(PA_NT == 4 * 64, "proto_apply_kernel: one wave per term array");

constexpr int PU_NW = PR_D / 64;  // waves of the update's block: a thread per feature

__global__ __launch_bounds__(PR_D) void proto_update_kernel(const float* __restrict__ bank, const int64_t* __restrict__ labels,
                                                           int64_t N, float* __restrict__ P, int n, double momentum, int first,
                                                           int64_t* __restrict__ count, int64_t* __restrict__ info) {
    __shared__ int rows[PR_D];   // the chunk's rows of class c, ascending (offsets into the chunk)
    __shared__ int wcnt[PU_NW];
    __shared__ unsigned long long hist[HB_MAXN + 1];  // block 0: rows per class, [n] = rows of no class
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool census = c == 0;
    if (census) {
        for (int j = t; j <= n; j += PR_D) hist[j] = 0ull;
        __syncthreads();
    }
    double acc = 0.0;
    int64_t cnt = 0;
    for (int64_t i0 = 0; i0 < N; i0 += PR_D) {
        const int64_t i = i0 + t;
        const int64_t lab = i < N ? labels[i] : (int64_t)-1;
        if (census && i < N) atomicAdd(&hist[(lab >= 0 && lab < n) ? (int)lab : n], 1ull);  // (integers: any order, one result)
        const bool mine = i < N && lab == (int64_t)c;
        const unsigned long long mask = __ballot(mine);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PU_NW; ++w) {
            if (w < wave) base += wcnt[w];
            total += wcnt[w];
        }
        if (mine) rows[base + __popcll(mask & ((1ull << lane) - 1ull))] = t;
        __syncthreads();
        const float* __restrict__ src = bank + (size_t)i0 * PR_D + t;
        int m = 0;
        for (; m + 4 <= total; m += 4) {  // four rows in flight, added in row order
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = src[(size_t)rows[m + e] * PR_D];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)r[e];
        }
        for (; m < total; ++m) acc += (double)src[(size_t)rows[m] * PR_D];
        cnt += total;
        __syncthreads();  // (rows / wcnt are rewritten by the next chunk)
    }
    if (cnt > 0) {
        const double mean = acc / (double)cnt;
        const size_t o = (size_t)c * PR_D + t;
        P[o] = (float)(first ? mean : (1.0 - momentum) * (double)P[o] + momentum * mean);
    }
    if (t == 0) count[c] = cnt;
    if (census && t == 0) {  // (behind the loop's last barrier: the histogram is complete)
        int64_t empty = 0;
        for (int j = 0; j < n; ++j) empty += hist[j] == 0ull;
        info[0] = empty;
        info[1] = (int64_t)hist[n];
    }
}

int proto_ce(const float* f, const float* P, const int64_t* labels, float* u, float* terms, float* sim, int B, int n, hipStream_t st) {
    hipLaunchKernelGGL(proto_ce_kernel, dim3(B), dim3(1024), 0, st, f, P, labels, u, terms, sim, B, n);
    GDL_CHECK_LAUNCH("proto_ce_kernel");
    return GDL_OK;
}

int proto_apply(const float* terms_a, const float* terms_v, const float* u_a, const float* u_v, float* dfa, float* dfv, float alpha,
                float* stats, int B, hipStream_t st) {
    hipLaunchKernelGGL(proto_apply_kernel, dim3(ceil_div(B * (PR_D / 4), PA_NT)), dim3(PA_NT), 0, st, terms_a, terms_v,
                       (const float4*)u_a, (const float4*)u_v, (float4*)dfa, (float4*)dfv, alpha, stats, B);
    GDL_CHECK_LAUNCH("proto_apply_kernel");
    return GDL_OK;
}

int proto_update(const float* bank, const int64_t* labels, int64_t N, float* P, int n, double momentum, int first, int64_t* count,
                 int64_t* info, hipStream_t st) {
    hipLaunchKernelGGL(proto_update_kernel, dim3(n), dim3(PR_D), 0, st, bank, labels, N, P, n, momentum, first, count, info);
    GDL_CHECK_LAUNCH("proto_update_kernel");
    return GDL_OK;
}

}  // namespace gdl
