// optim.hip -- fused multi-tensor gradient statistics, clipping and SGD over flat arenas.
//
// Replaces, for the step of /root/reference/main_dgl.py:
//   nn.utils.clip_grad_norm_(model.parameters(), max_norm=40, norm_type=2)      (:129)
//   sum_p torch.abs(p.grad).mean() over audio_net / visual_net parameters        (:132-143)
//   optim.SGD(lr, momentum=0.9, weight_decay=1e-4).step()                        (:249,154)
// which the reference runs as ~370 small launches and 120 host syncs.  Here: one pass over
// the gradient arena (sum of squares + sum of |g| per parameter, fixed-order reduction in
// double), one tiny finalise kernel that leaves {total_norm, clip_coef, audio_sum,
// visual_sum, per-parameter norms} on the device, and one streaming update kernel.
#include "common.h"
#include "philox.h"
#include "prof.h"

#include <string.h>

#include <vector>

struct gdl_optim {
    int nseg = 0;
    int64_t total = 0;
    int nchunks = 0;
    std::vector<int64_t> offs;
    std::vector<int32_t> group;
    // The object owns NO device memory (the library never allocates or frees device memory).  Its descriptor
    // tables -- chunk descriptors ChunkDesc[nchunks], per-segment chunk ranges int32[nseg][4] = {first_chunk, n_chunks, group, 0},
    // per-segment element counts double[nseg] -- are kept on the host and uploaded into the head of the caller-provided
    // workspace the first time gdl_optim_grad_stats sees that workspace (stream-ordered, once per workspace pointer):
    //   ws = [chunk descriptors | segment ranges | element counts | per-chunk partials | per-segment sums]
    std::vector<unsigned char> h_tables;  // the first three, concatenated as they sit in the workspace
    size_t off_segrange = 0, off_segnumel = 0, off_partial = 0;
    const void* bound_ws = nullptr;
    // gradient modulation (OGM / OGM-GE): per-segment marks 0 = untouched, 1 = audio, 2 = visual, kept on the host and uploaded
    // into the head of the caller's modulation workspace by gdl_optim_modulate_bind: mod_ws = [marks int32[nseg] | per-chunk sums]
    std::vector<int32_t> marks;
    size_t off_modpartial = 0;
    const void* bound_mod_ws = nullptr;
};

namespace gdl {

constexpr int OPT_CHUNK = 8192;

struct ChunkDesc {
    int64_t start;
    int32_t len;
    int32_t seg;
};

__global__ __launch_bounds__(256) void grad_stats_kernel(const float* __restrict__ g, const ChunkDesc* __restrict__ chunks,
                                                         double* __restrict__ partial) {
    __shared__ double sh[2][256];
    const ChunkDesc c = chunks[blockIdx.x];
    const float* p = g + c.start;
    float s2 = 0.f, s1 = 0.f;
    // 16-byte loads over the aligned middle of the chunk (segments start at arbitrary element offsets), scalar ends
    const int head = min(c.len, (int)((4 - (c.start & 3)) & 3));
    const int nv = (c.len - head) >> 2;
    const float4* p4 = (const float4*)(p + head);
    for (int i = threadIdx.x; i < nv; i += 256) {
        const float4 v = p4[i];
        s2 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        s1 += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
    }
    {  // at most 3 elements in front of and 3 behind the aligned middle
        const int i = (int)threadIdx.x < head ? (int)threadIdx.x : head + 4 * nv + ((int)threadIdx.x - head);
        if (i < c.len && ((int)threadIdx.x < head || (int)threadIdx.x - head < c.len - head - 4 * nv)) {
            const float v = p[i];
            s2 += v * v;
            s1 += fabsf(v);
        }
    }
    sh[0][threadIdx.x] = (double)s2;
    sh[1][threadIdx.x] = (double)s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * 2 + 0] = sh[0][0];
        partial[(size_t)blockIdx.x * 2 + 1] = sh[1][0];
    }
}

// stats[0] total_norm (pre-clip, after grad_scale), [1] clip_coef, [2] audio_sum, [3] visual_sum,
// [4+s] post-clip L2 norm of segment s, [4+nseg+s] post-clip mean|g| of segment s.
constexpr int FIN_NT = 1024;
__global__ __launch_bounds__(FIN_NT) void grad_stats_final_kernel(const double* __restrict__ partial,
                                                               const int32_t* __restrict__ segrange,
                                                               const double* __restrict__ segnumel, int nseg,
                                                               float max_norm, float grad_scale, float* __restrict__ stats,
                                                               double* __restrict__ segsum /*[nseg][2] scratch*/) {
    __shared__ double sh[3][FIN_NT];
    // A 16-lane group per segment (a layer-4 convolution has 288 chunk partials: one thread adding them serially
    // took 47 us): lane l adds chunks l, l+16, ..., the 16 lanes are folded in a fixed order.  Round 5: 1024 threads = 64 groups
    // (the 122 segments in two rounds instead of eight: this launch sits alone between the last gradient and the update, 18 us).
    const int grp16 = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    for (int s = grp16; s < nseg; s += FIN_NT / 16) {
        const int first = segrange[s * 4 + 0], cnt = segrange[s * 4 + 1];
        double a = 0.0, b = 0.0;
        for (int k = l16; k < cnt; k += 16) {
            a += partial[(size_t)(first + k) * 2 + 0];
            b += partial[(size_t)(first + k) * 2 + 1];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            a += __shfl_down(a, o, 16);
            b += __shfl_down(b, o, 16);
        }
        if (l16 == 0) {
            segsum[s * 2 + 0] = a;
            segsum[s * 2 + 1] = b;
        }
    }
    __syncthreads();  // (segsum is global memory written and read by this one block)
    double tot = 0.0;
    for (int s = threadIdx.x; s < nseg; s += FIN_NT) tot += segsum[s * 2 + 0];
    sh[0][threadIdx.x] = tot;
    __syncthreads();
    for (int o = FIN_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
        __syncthreads();
    }
    const double norm = sqrt(sh[0][0]) * (double)grad_scale;
    // torch: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (float arithmetic there; double here)
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    __syncthreads();
    double au = 0.0, vi = 0.0;
    for (int s = threadIdx.x; s < nseg; s += FIN_NT) {
        const double l2 = sqrt(segsum[s * 2 + 0]) * (double)grad_scale * coef;
        const double am = segsum[s * 2 + 1] / segnumel[s] * (double)grad_scale * coef;
        stats[4 + s] = (float)l2;
        stats[4 + nseg + s] = (float)am;
        const int grp = segrange[s * 4 + 2];
        if (grp == 1) au += am;
        if (grp == 2) vi += am;
    }
    sh[1][threadIdx.x] = au;
    sh[2][threadIdx.x] = vi;
    __syncthreads();
    for (int o = FIN_NT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = (float)norm;
        stats[1] = (float)coef;
        stats[2] = (float)sh[1][0];
        stats[3] = (float)sh[2][0];
    }
}

// g *= coef*grad_scale (stored back: p.grad is clipped in place by the reference);
// d = g + wd*p; m = mu*m + d; p -= lr*m
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                  const float* __restrict__ stats, float grad_scale, float lr, float mu,
                                                  float wd, int64_t n) {
    const float k = (stats ? stats[1] : 1.f) * grad_scale;
    const bool wb = k != 1.f;  // (clip inactive on one rank: g * 1 is g -- its 4 n bytes are not written back)
    const int64_t nv = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        float4 pv = ((float4*)p)[i], gv = ((float4*)g)[i], mv = ((float4*)m)[i];
        gv.x *= k;
        gv.y *= k;
        gv.z *= k;
        gv.w *= k;
        mv.x = mu * mv.x + (gv.x + wd * pv.x);
        mv.y = mu * mv.y + (gv.y + wd * pv.y);
        mv.z = mu * mv.z + (gv.z + wd * pv.z);
        mv.w = mu * mv.w + (gv.w + wd * pv.w);
        pv.x -= lr * mv.x;
        pv.y -= lr * mv.y;
        pv.z -= lr * mv.z;
        pv.w -= lr * mv.w;
        if (wb) ((float4*)g)[i] = gv;
        ((float4*)m)[i] = mv;
        ((float4*)p)[i] = pv;
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += 256) {
            const float gg = g[i] * k;
            const float mm = mu * m[i] + (gg + wd * p[i]);
            if (wb) g[i] = gg;
            m[i] = mm;
            p[i] -= lr * mm;
        }
    }
}

// torch.optim.AdamW (_single_tensor_adam, decoupled weight decay) for one element, in torch's order of operations:
// p *= 1 - lr*wd; m = lerp(m, g, 1 - beta1); v = beta2*v + (1 - beta2)*g*g; p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
struct AdamWScalars {
    float decay, b1c, beta2, b2c, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamWScalars& s) {
    p *= s.decay;
    m += s.b1c * (g - m);
    v = s.beta2 * v + s.b2c * (g * g);
    p -= s.step_size * (m / (sqrtf(v) / s.bc2_sqrt + s.eps));
}

// g *= coef*grad_scale (stored back only when that is not 1, as sgd_kernel), then adamw1
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, const float* __restrict__ stats, float grad_scale,
                                                    AdamWScalars s, int64_t n) {
    const float k = (stats ? stats[1] : 1.f) * grad_scale;
    const bool wb = k != 1.f;
    const int64_t nv = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        float4 pv = ((float4*)p)[i], gv = ((float4*)g)[i], mv = ((float4*)m)[i], vv = ((float4*)v)[i];
        gv.x *= k;
        gv.y *= k;
        gv.z *= k;
        gv.w *= k;
        adamw1(pv.x, gv.x, mv.x, vv.x, s);
        adamw1(pv.y, gv.y, mv.y, vv.y, s);
        adamw1(pv.z, gv.z, mv.z, vv.z, s);
        adamw1(pv.w, gv.w, mv.w, vv.w, s);
        if (wb) ((float4*)g)[i] = gv;
        ((float4*)m)[i] = mv;
        ((float4*)v)[i] = vv;
        ((float4*)p)[i] = pv;
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += 256) {
            const float gg = g[i] * k;
            float pp = p[i], mm = m[i], ss = v[i];
            adamw1(pp, gg, mm, ss, s);
            if (wb) g[i] = gg;
            m[i] = mm;
            v[i] = ss;
            p[i] = pp;
        }
    }
}

// torch.optim.Adagrad (_single_tensor_adagrad, lr_decay 0) for one element: d = g + wd*p (a temporary, as torch's
// grad.add(param, alpha=wd) is); s += d*d; p -= lr * d / (sqrt(s) + eps)
__device__ __forceinline__ void adagrad1(float& p, float g, float& s, float lr, float eps, float wd) {
    const float d = g + wd * p;
    s += d * d;
    p -= lr * (d / (sqrtf(s) + eps));
}

__global__ __launch_bounds__(256) void adagrad_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ sum,
                                                      const float* __restrict__ stats, float grad_scale, float lr, float eps,
                                                      float wd, int64_t n) {
    const float k = (stats ? stats[1] : 1.f) * grad_scale;
    const bool wb = k != 1.f;
    const int64_t nv = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        float4 pv = ((float4*)p)[i], gv = ((float4*)g)[i], sv = ((float4*)sum)[i];
        gv.x *= k;
        gv.y *= k;
        gv.z *= k;
        gv.w *= k;
        adagrad1(pv.x, gv.x, sv.x, lr, eps, wd);
        adagrad1(pv.y, gv.y, sv.y, lr, eps, wd);
        adagrad1(pv.z, gv.z, sv.z, lr, eps, wd);
        adagrad1(pv.w, gv.w, sv.w, lr, eps, wd);
        if (wb) ((float4*)g)[i] = gv;
        ((float4*)sum)[i] = sv;
        ((float4*)p)[i] = pv;
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += 256) {
            const float gg = g[i] * k;
            float pp = p[i], ss = sum[i];
            adagrad1(pp, gg, ss, lr, eps, wd);
            if (wb) g[i] = gg;
            sum[i] = ss;
            p[i] = pp;
        }
    }
}

// ---------------------------------------------------------------- OGM / OGM-GE gradient modulation (main.py:286-330)
// Between the clip and the update, for every marked segment (the 4-D tensors of an encoder) with c its modality's coefficient:
//   OGM:    g <- (g k) c                       k = clip_coef * grad_scale, what the update kernels multiply by
//   OGM_GE: g <- (g k) c + sigma z             sigma = std(g k) + 1e-8 (unbiased, of the whole clipped tensor), z ~ N(0, 1)
// Unmarked segments get g k, as the update kernels would have written it; those then run with stats = NULL, grad_scale = 1.
// Three launches: the per-chunk sum of the marked chunks (the statistics pass has the sum of squares), one block that turns
// the scores into the two coefficients and the sums into the per-segment sigma, and the chunked in-place pass.

// (the generator -- Philox4x32-10, Box-Muller and noise4, the keying by arena element -- is in philox.h)

// sum of g over each chunk of a marked segment (float per thread over at most 32 elements, then double, in a fixed order)
__global__ __launch_bounds__(256) void mod_sum_kernel(const float* __restrict__ g, const ChunkDesc* __restrict__ chunks,
                                                      const int32_t* __restrict__ marks, double* __restrict__ partial) {
    __shared__ double sh[256];
    const ChunkDesc c = chunks[blockIdx.x];
    if (marks[c.seg] == 0) return;
    const float* p = g + c.start;
    float s = 0.f;
    const int head = min(c.len, (int)((4 - (c.start & 3)) & 3));
    const int nv = (c.len - head) >> 2;
    const float4* p4 = (const float4*)(p + head);
    for (int i = threadIdx.x; i < nv; i += 256) {
        const float4 v = p4[i];
        s += (v.x + v.y) + (v.z + v.w);
    }
    {  // the at most 3 + 3 elements around the aligned middle
        const int t = threadIdx.x, tail = c.len - head - 4 * nv;
        if (t < head) s += p[t];
        else if (t - head < tail) s += p[head + 4 * nv + (t - head)];
    }
    sh[threadIdx.x] = (double)s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// mstats[0] score_a, [1] score_v, [2] ratio_v, [3] coeff_a, [4] coeff_v, [5..7] 0, [8 + s] sigma of segment s (0 where unmarked
// or without noise).  segsum: the statistics pass's per-segment {sum g^2, sum |g|} of the unscaled gradient.
constexpr int MOD_STATS_HEAD = 8;
__global__ __launch_bounds__(FIN_NT) void mod_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ segrange,
                                                        const double* __restrict__ segnumel, const int32_t* __restrict__ marks,
                                                        const double* __restrict__ segsum, int nseg,
                                                        const float* __restrict__ stats, float grad_scale,
                                                        const float* __restrict__ scores, float alpha, int noise,
                                                        float* __restrict__ mstats) {
    const float k = stats[1] * grad_scale;  // the update kernels' factor, in their arithmetic
    const int grp16 = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    for (int s = grp16; s < nseg; s += FIN_NT / 16) {  // (the 16-lane fold of grad_stats_final_kernel)
        float sigma = 0.f;
        if (noise && marks[s] != 0) {
            const int first = segrange[s * 4 + 0], cnt = segrange[s * 4 + 1];
            double a = 0.0;
            for (int j = l16; j < cnt; j += 16) a += partial[first + j];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) a += __shfl_down(a, o, 16);
            const double n = segnumel[s];
            double var = (segsum[s * 2 + 0] - a * a / n) / (n - 1.0);
            if (var < 0.0) var = 0.0;
            sigma = (float)((double)k * sqrt(var) + 1e-8);
        }
        if (l16 == 0) mstats[MOD_STATS_HEAD + s] = sigma;
    }
    if (threadIdx.x == 0) {
        // ratio_v = score_v / score_a; the side that leads is slowed by 1 - tanh(alpha * its ratio) (= 2 / (e^2x + 1): no
        // cancellation), the other keeps 1; ratio_v == 1 takes the audio branch (main.py:296-301)
        const double sa = (double)scores[0], sv = (double)scores[1];
        const double rv = sv / sa;
        double ca = 1.0, cv = 1.0;
        if (rv > 1.0)
            cv = 2.0 / (exp(2.0 * (double)alpha * rv) + 1.0);
        else
            ca = 2.0 / (exp(2.0 * (double)alpha * (1.0 / rv)) + 1.0);
        mstats[0] = scores[0];
        mstats[1] = scores[1];
        mstats[2] = (float)rv;
        mstats[3] = (float)ca;
        mstats[4] = (float)cv;
        mstats[5] = mstats[6] = mstats[7] = 0.f;
    }
}

template <bool NOISE>
__device__ __forceinline__ float mod1(float g, float k, float c, float sigma, float z) {
    const float gk = g * k;
    return NOISE ? fmaf(sigma, z, gk * c) : gk * c;
}

// one chunk per block, in place; element i of the arena takes the normal z[i & 3] of its aligned group of four
template <bool NOISE>
__global__ __launch_bounds__(256) void modulate_kernel(float* __restrict__ g, const ChunkDesc* __restrict__ chunks,
                                                       const int32_t* __restrict__ marks, const float* __restrict__ stats,
                                                       float grad_scale, const float* __restrict__ mstats, uint32_t seed_lo,
                                                       uint32_t seed_hi, int64_t step) {
    const ChunkDesc c = chunks[blockIdx.x];
    const float k = stats[1] * grad_scale;
    const int mark = marks[c.seg];
    float* p = g + c.start;
    const int head = min(c.len, (int)((4 - (c.start & 3)) & 3));
    const int nv = (c.len - head) >> 2;
    float4* p4 = (float4*)(p + head);
    if (mark == 0) {  // g k, stored only where the update kernels would have stored it
        if (k == 1.f) return;
        for (int i = threadIdx.x; i < nv; i += 256) {
            float4 v = p4[i];
            v.x *= k;
            v.y *= k;
            v.z *= k;
            v.w *= k;
            p4[i] = v;
        }
        const int t = threadIdx.x, tail = c.len - head - 4 * nv;
        if (t < head) p[t] *= k;
        else if (t - head < tail) p[head + 4 * nv + (t - head)] *= k;
        return;
    }
    const float coef = mstats[2 + mark];  // [3] audio, [4] visual
    const float sigma = NOISE ? mstats[MOD_STATS_HEAD + c.seg] : 0.f;
    const int64_t q0 = (c.start + head) >> 2;
    for (int i = threadIdx.x; i < nv; i += 256) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE) noise4(q0 + i, step, seed_lo, seed_hi, z);
        float4 v = p4[i];
        v.x = mod1<NOISE>(v.x, k, coef, sigma, z[0]);
        v.y = mod1<NOISE>(v.y, k, coef, sigma, z[1]);
        v.z = mod1<NOISE>(v.z, k, coef, sigma, z[2]);
        v.w = mod1<NOISE>(v.w, k, coef, sigma, z[3]);
        p4[i] = v;
    }
    {
        const int t = threadIdx.x, tail = c.len - head - 4 * nv;
        const int j = t < head ? t : (t - head < tail ? head + 4 * nv + (t - head) : -1);
        if (j >= 0) {
            const int64_t e = c.start + j;
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (NOISE) noise4(e >> 2, step, seed_lo, seed_hi, z);
            const int l = (int)(e & 3);
            p[j] = mod1<NOISE>(p[j], k, coef, sigma, l == 0 ? z[0] : (l == 1 ? z[1] : (l == 2 ? z[2] : z[3])));
        }
    }
}

// grid of the streaming update kernels: one float4 per thread, grid-stride beyond 4096 blocks of 256
static int64_t update_blocks(int64_t total) {
    int64_t blocks = ((total >> 2) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    return blocks;
}

}  // namespace gdl

using namespace gdl;

extern "C" {

int gdl_optim_create(gdl_optim_t** out, const int64_t* seg_offsets, const int32_t* seg_group, int nseg) {
    GDL_REQUIRE(out && seg_offsets && seg_group && nseg > 0, "optim_create: bad arguments");
    GDL_REQUIRE(seg_offsets[0] == 0, "optim_create: arena must start at offset 0");
    gdl_optim* o = new gdl_optim();
    o->nseg = nseg;
    o->offs.assign(seg_offsets, seg_offsets + nseg + 1);
    o->group.assign(seg_group, seg_group + nseg);
    o->total = seg_offsets[nseg];
    std::vector<ChunkDesc> chunks;
    std::vector<int32_t> segrange(nseg * 4);
    std::vector<double> numel(nseg);
    for (int s = 0; s < nseg; ++s) {
        const int64_t b = seg_offsets[s], e = seg_offsets[s + 1];
        if (e <= b) {
            delete o;
            set_error("optim_create: empty or unordered segment %d", s);
            return GDL_ERR_ARG;
        }
        segrange[s * 4 + 0] = (int32_t)chunks.size();
        for (int64_t c = b; c < e; c += OPT_CHUNK) {
            ChunkDesc d;
            d.start = c;
            d.len = (int32_t)((e - c) < OPT_CHUNK ? (e - c) : OPT_CHUNK);
            d.seg = s;
            chunks.push_back(d);
        }
        segrange[s * 4 + 1] = (int32_t)chunks.size() - segrange[s * 4 + 0];
        segrange[s * 4 + 2] = seg_group[s];
        segrange[s * 4 + 3] = 0;
        numel[s] = (double)(e - b);
    }
    o->nchunks = (int)chunks.size();
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    o->off_segrange = up(chunks.size() * sizeof(ChunkDesc));
    o->off_segnumel = up(o->off_segrange + segrange.size() * sizeof(int32_t));
    o->off_partial = up(o->off_segnumel + numel.size() * sizeof(double));
    o->h_tables.assign(o->off_partial, 0);
    memcpy(o->h_tables.data(), chunks.data(), chunks.size() * sizeof(ChunkDesc));
    memcpy(o->h_tables.data() + o->off_segrange, segrange.data(), segrange.size() * sizeof(int32_t));
    memcpy(o->h_tables.data() + o->off_segnumel, numel.data(), numel.size() * sizeof(double));
    *out = o;
    return GDL_OK;
}

void gdl_optim_destroy(gdl_optim_t* o) { delete o; }

size_t gdl_optim_workspace_bytes(const gdl_optim_t* o) {
    if (!o) return 0;
    return o->off_partial + ((size_t)o->nchunks * 2 + (size_t)o->nseg * 2) * sizeof(double);
}

int gdl_optim_stats_len(const gdl_optim_t* o) { return o ? 4 + 2 * o->nseg : 0; }

int gdl_optim_bind_workspace(gdl_optim_t* o, void* ws, size_t ws_bytes, void* stream) {
    GDL_REQUIRE(o && ws, "optim_bind_workspace: null argument");
    if (ws_bytes < gdl_optim_workspace_bytes(o)) {
        set_error("optim_bind_workspace: workspace %zu < %zu", ws_bytes, gdl_optim_workspace_bytes(o));
        return GDL_ERR_WORKSPACE;
    }
    GDL_REQUIRE(((uintptr_t)ws & 15) == 0, "optim_bind_workspace: workspace must be 16-byte aligned");
    hipError_t he = hipMemcpyAsync(ws, o->h_tables.data(), o->h_tables.size(), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he != hipSuccess) return check_hip(he, "optim_bind_workspace: descriptor upload");
    o->bound_ws = ws;
    return GDL_OK;
}

int gdl_optim_grad_stats(gdl_optim_t* o, const float* grads, float max_norm, float grad_scale, float* stats, void* ws,
                         size_t ws_bytes, void* stream) {
    GDL_REQUIRE(o && grads && stats && ws, "optim_grad_stats: null argument");
    if (ws_bytes < gdl_optim_workspace_bytes(o)) {
        set_error("optim_grad_stats: workspace %zu < %zu", ws_bytes, gdl_optim_workspace_bytes(o));
        return GDL_ERR_WORKSPACE;
    }
    GDL_REQUIRE(((uintptr_t)ws & 15) == 0, "optim_grad_stats: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)ws;
    if (o->bound_ws != ws) {  // descriptor tables -> the head of this workspace (once; ordered on `stream` like the kernels)
        hipError_t he = hipMemcpyAsync(w, o->h_tables.data(), o->h_tables.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return check_hip(he, "optim_grad_stats: descriptor upload");
        o->bound_ws = ws;
    }
    double* partial = (double*)(w + o->off_partial);
    double* segsum = partial + (size_t)o->nchunks * 2;
    {
        ProfScope prof("gdl::grad_stats_kernel", PROF_HBM, st, (double)o->total * 4.0);
        hipLaunchKernelGGL(grad_stats_kernel, dim3(o->nchunks), dim3(256), 0, st, grads, (const ChunkDesc*)w, partial);
    }
    GDL_CHECK_LAUNCH("grad_stats_kernel");
    hipLaunchKernelGGL(grad_stats_final_kernel, dim3(1), dim3(FIN_NT), 0, st, (const double*)partial,
                       (const int32_t*)(w + o->off_segrange), (const double*)(w + o->off_segnumel), o->nseg, max_norm, grad_scale,
                       stats, segsum);
    GDL_CHECK_LAUNCH("grad_stats_final_kernel");
    return GDL_OK;
}

size_t gdl_optim_modulate_workspace_bytes(const gdl_optim_t* o) {
    if (!o) return 0;
    return (((size_t)o->nseg * sizeof(int32_t) + 255) & ~(size_t)255) + (size_t)o->nchunks * sizeof(double);
}

int gdl_optim_modulate_stats_len(const gdl_optim_t* o) { return o ? MOD_STATS_HEAD + o->nseg : 0; }

int gdl_optim_modulate_bind(gdl_optim_t* o, const int32_t* seg_mark, void* mod_ws, size_t mod_ws_bytes, void* stream) {
    GDL_REQUIRE(o && seg_mark && mod_ws, "optim_modulate_bind: null argument");
    if (mod_ws_bytes < gdl_optim_modulate_workspace_bytes(o)) {
        set_error("optim_modulate_bind: workspace %zu < %zu", mod_ws_bytes, gdl_optim_modulate_workspace_bytes(o));
        return GDL_ERR_WORKSPACE;
    }
    GDL_REQUIRE(((uintptr_t)mod_ws & 15) == 0, "optim_modulate_bind: workspace must be 16-byte aligned");
    for (int s = 0; s < o->nseg; ++s) {
        GDL_REQUIRE(seg_mark[s] >= 0 && seg_mark[s] <= 2, "optim_modulate_bind: mark %d of segment %d (0 untouched, 1 audio, 2 visual)",
                    seg_mark[s], s);
        // (the unbiased standard deviation divides by n - 1)
        GDL_REQUIRE(seg_mark[s] == 0 || o->offs[s + 1] - o->offs[s] >= 2, "optim_modulate_bind: marked segment %d has fewer than 2 elements", s);
    }
    o->marks.assign(seg_mark, seg_mark + o->nseg);
    o->off_modpartial = ((size_t)o->nseg * sizeof(int32_t) + 255) & ~(size_t)255;
    hipError_t he = hipMemcpyAsync(mod_ws, o->marks.data(), o->marks.size() * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he != hipSuccess) return check_hip(he, "optim_modulate_bind: mark upload");
    o->bound_mod_ws = mod_ws;
    return GDL_OK;
}

int gdl_optim_modulate(gdl_optim_t* o, float* grads, const float* stats, float grad_scale, const float* scores, float alpha,
                       int noise, int64_t seed, int64_t step, float* mod_stats, const void* ws, void* mod_ws, void* stream) {
    GDL_REQUIRE(o && grads && stats && scores && mod_stats && ws && mod_ws, "optim_modulate: null argument");
    GDL_REQUIRE(noise == 0 || noise == 1, "optim_modulate: noise must be 0 (OGM) or 1 (OGM_GE)");
    GDL_REQUIRE(((uintptr_t)grads & 15) == 0, "optim_modulate: the gradient arena must be 16-byte aligned");
    GDL_REQUIRE(o->bound_mod_ws == mod_ws && !o->marks.empty(), "optim_modulate: mod_ws is not the workspace gdl_optim_modulate_bind was given");
    GDL_REQUIRE(o->bound_ws == ws, "optim_modulate: ws is not the workspace gdl_optim_grad_stats last ran on");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* w = (const unsigned char*)ws;
    const ChunkDesc* chunks = (const ChunkDesc*)w;
    const int32_t* segrange = (const int32_t*)(w + o->off_segrange);
    const double* segnumel = (const double*)(w + o->off_segnumel);
    const double* segsum = (const double*)(w + o->off_partial) + (size_t)o->nchunks * 2;
    const int32_t* marks = (const int32_t*)mod_ws;
    double* partial = (double*)((unsigned char*)mod_ws + o->off_modpartial);
    int64_t marked = 0;
    for (int s = 0; s < o->nseg; ++s)
        if (o->marks[s]) marked += o->offs[s + 1] - o->offs[s];
    if (noise) {
        ProfScope prof("gdl::mod_sum_kernel", PROF_HBM, st, (double)marked * 4.0);
        hipLaunchKernelGGL(mod_sum_kernel, dim3(o->nchunks), dim3(256), 0, st, (const float*)grads, chunks, marks, partial);
        GDL_CHECK_LAUNCH("mod_sum_kernel");
    }
    hipLaunchKernelGGL(mod_final_kernel, dim3(1), dim3(FIN_NT), 0, st, (const double*)partial, segrange, segnumel, marks, segsum,
                       o->nseg, stats, grad_scale, scores, alpha, noise, mod_stats);
    GDL_CHECK_LAUNCH("mod_final_kernel");
    {
        // (marked elements read and written; the unmarked ones only where clip_coef * grad_scale != 1, not charged -- as sgd_kernel)
        ProfScope prof(noise ? "gdl::modulate_kernel<true>" : "gdl::modulate_kernel<false>", PROF_HBM, st, (double)marked * 8.0);
        if (noise)
            hipLaunchKernelGGL(modulate_kernel<true>, dim3(o->nchunks), dim3(256), 0, st, grads, chunks, marks, stats, grad_scale,
                               (const float*)mod_stats, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), step);
        else
            hipLaunchKernelGGL(modulate_kernel<false>, dim3(o->nchunks), dim3(256), 0, st, grads, chunks, marks, stats, grad_scale,
                               (const float*)mod_stats, 0u, 0u, step);
        GDL_CHECK_LAUNCH("modulate_kernel");
    }
    return GDL_OK;
}

int gdl_optim_sgd_step(gdl_optim_t* o, float* params, float* grads, float* momentum, const float* stats, float grad_scale,
                       float lr, float mu, float wd, void* stream) {
    GDL_REQUIRE(o && params && grads && momentum, "optim_sgd_step: null argument");
    GDL_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum) & 15) == 0,
                "optim_sgd_step: arenas must be 16-byte aligned");
    const int64_t nv = o->total >> 2;
    int64_t blocks = (nv + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    // (p, g, m read + p, m written = 20 n bytes; the clipped gradient's 4 n-byte write-back only happens when the clip is active --
    // decided on the device, stats[1] -- and is not charged: round 3's 24 n overstated the kernel at 0.96 of the HBM peak)
    ProfScope prof("gdl::sgd_kernel", PROF_HBM, (hipStream_t)stream, (double)o->total * 4.0 * 5);
    hipLaunchKernelGGL(sgd_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, params, grads, momentum, stats,
                       grad_scale, lr, mu, wd, o->total);
    GDL_CHECK_LAUNCH("sgd_kernel");
    return GDL_OK;
}

// The hyperparameters arrive as doubles, the values torch.optim holds: the per-step scalars are derived from them in double
// and rounded once, as torch rounds a Python scalar into a float32 tensor operation (a float 0.999 alone would move 1 - beta2,
// the weight of the second moment, by 1.3e-5 relative).
int gdl_optim_adamw_step(gdl_optim_t* o, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* stats,
                         float grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                         void* stream) {
    GDL_REQUIRE(o && params && grads && exp_avg && exp_avg_sq, "optim_adamw_step: null argument");
    GDL_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                "optim_adamw_step: arenas must be 16-byte aligned");
    GDL_REQUIRE(step >= 1, "optim_adamw_step: step must be >= 1 (the bias corrections count from 1)");
    AdamWScalars s;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.b1c = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.b2c = (float)(1.0 - beta2);
    s.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    s.eps = (float)eps;
    // (p, g, m, v read + p, m, v written = 28 n bytes; the conditional gradient write-back is not charged, as for SGD)
    ProfScope prof("gdl::adamw_kernel", PROF_HBM, (hipStream_t)stream, (double)o->total * 4.0 * 7);
    hipLaunchKernelGGL(adamw_kernel, dim3((int)update_blocks(o->total)), dim3(256), 0, (hipStream_t)stream, params, grads,
                       exp_avg, exp_avg_sq, stats, grad_scale, s, o->total);
    GDL_CHECK_LAUNCH("adamw_kernel");
    return GDL_OK;
}

int gdl_optim_adagrad_step(gdl_optim_t* o, float* params, float* grads, float* state_sum, const float* stats, float grad_scale,
                           double lr, double eps, double weight_decay, int64_t step, void* stream) {
    GDL_REQUIRE(o && params && grads && state_sum, "optim_adagrad_step: null argument");
    GDL_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)state_sum) & 15) == 0,
                "optim_adagrad_step: arenas must be 16-byte aligned");
    GDL_REQUIRE(step >= 1, "optim_adagrad_step: step must be >= 1");
    // (p, g, s read + p, s written = 20 n bytes)
    ProfScope prof("gdl::adagrad_kernel", PROF_HBM, (hipStream_t)stream, (double)o->total * 4.0 * 5);
    hipLaunchKernelGGL(adagrad_kernel, dim3((int)update_blocks(o->total)), dim3(256), 0, (hipStream_t)stream, params, grads,
                       state_sum, stats, grad_scale, (float)lr, (float)eps, (float)weight_decay, o->total);
    GDL_CHECK_LAUNCH("adagrad_kernel");
    return GDL_OK;
}

}  // extern "C"
