// dul.hip -- the probabilistic-embedding branch of main.py (--pe 1 --beta b): the two Conv2d(1x1) + BatchNorm2d stacks
// mu_dul_backbone / logvar_dul_backbone behind an encoder's final map (models/swin_transformer.py:574-582, :643-667; the
// ResNet of the scripts carries the same two stacks), the reparameterised sample, the pooled feature and the KL term `regurize`
// (main.py:92-102, :191-213).  The 1x1 products and the BatchNorm statistics are the existing entry points' (gdl_conv_fwd_bias,
// gdl_bn_stats, gdl_bn_finalize_train, gdl_conv_dgrad, gdl_conv_wgrad, gdl_bn_bwd_finalize); this file holds what lies between
// them.  All arithmetic is float32 whatever the storage type of z (a bf16 map is widened on load).
//
// With z_mu, z_lv [M][512] the two convolutions' outputs (M = n_img P rows, row r of sample b = r / (T P)), and per stack
// bn = float [4][512] = {scale, shift, save_mean, save_rstd} as gdl_bn_finalize_train leaves them:
//   mu = fmaf(z_mu, scale_mu, shift_mu)   lv = fmaf(z_lv, scale_lv, shift_lv)   sd = expf(0.5f lv)   out = fmaf(eps, sd, mu)
//   f[b][c]  = (sum over the sample's T P rows of out[r][c]) / (T P)
//   reg      = (sum over rows and channels of 0.5f (sd^2 + mu^2 - logf(sd^2 + 1e-8f) - 1)) / n_img
// eps: the caller's float32 [M][512] map, or dul_noise4 (philox.h) of (seed, step, modality, element index r 512 + c).
// Backward from df [B][512], k = beta / n_img, g = df[b][c] / (T P):
//   d_mu = g + k mu      d_sd = g eps + k (sd - sd / (sd^2 + 1e-8f))      d_lv = d_sd 0.5f sd
// then each stack's BatchNorm backward in the two-pass form of bn.hip: per-block partials of (sum d, sum d xhat),
// gdl_bn_bwd_finalize, and dz = gamma rstd (d - coef0 - xhat coef1) in the storage type the convolutions read.
//
// Fixed orders (run-to-run identical, no floating-point atomic, no block waits for another):
//   pool: a block owns one sample and 16 channel vectors; its 16 row-lanes take rows j = lane, lane + 16, ... of the sample in
//         ascending order, then the 16 lane sums are added in ascending lane order;
//   KL:   per thread in the same row order over its vector's channels, the block's 256 terms by the tree o = 128 .. 1, the
//         blocks' terms by ticket.h's last-block fold (ticket_fold256).
#include "common.h"
#include "ops.h"
#include "philox.h"
#include "prof.h"
#include "ticket.h"

namespace gdl {

constexpr int DUL_C = 512;   // channels
constexpr int DUL_NT = 256;  // threads
constexpr int DUL_CV = 16;   // sample kernel: channel vectors per block
constexpr int DUL_RL = DUL_NT / DUL_CV;  // row lanes

template <int EPC>
__device__ __forceinline__ void dul_ldf(const float* __restrict__ p, float (&v)[EPC]) {
#pragma unroll
    for (int q = 0; q < EPC / 4; ++q) {
        const float4 t = *(const float4*)(p + 4 * q);
        v[4 * q + 0] = t.x;
        v[4 * q + 1] = t.y;
        v[4 * q + 2] = t.z;
        v[4 * q + 3] = t.w;
    }
}
template <int EPC>
__device__ __forceinline__ void dul_stf(float* __restrict__ p, const float (&v)[EPC]) {
#pragma unroll
    for (int q = 0; q < EPC / 4; ++q) *(float4*)(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
template <typename T>
__device__ __forceinline__ void dul_ldz(const T* __restrict__ p, float (&v)[TT<T>::EPC]) {
    unpack16<T>(*(const uint4*)p, v);
}
// the normals of elements e0 .. e0 + EPC - 1 (e0 % EPC == 0): supplied, or drawn
template <int EPC>
__device__ __forceinline__ void dul_eps(const float* __restrict__ eps_in, size_t e0, int modality, int64_t step, uint32_t seed_lo,
                                        uint32_t seed_hi, float (&z)[EPC]) {
    if (eps_in) {
        dul_ldf<EPC>(eps_in + e0, z);
    } else {
#pragma unroll
        for (int q = 0; q < EPC / 4; ++q) {
            float n[4];
            dul_noise4((uint32_t)(e0 >> 2) + q, modality, step, seed_lo, seed_hi, n);
            z[4 * q + 0] = n[0], z[4 * q + 1] = n[1], z[4 * q + 2] = n[2], z[4 * q + 3] = n[3];
        }
    }
}

// ---------------------------------------------------------------- training forward
template <typename T, bool MAPS>
__global__ __launch_bounds__(DUL_NT) void dul_sample_kernel(const T* __restrict__ z_mu, const T* __restrict__ z_lv,
                                                            const float* __restrict__ bn_mu, const float* __restrict__ bn_lv,
                                                            const float* __restrict__ eps_in, uint32_t seed_lo, uint32_t seed_hi,
                                                            int64_t step, int modality, float* __restrict__ f,
                                                            float* __restrict__ reg, float* __restrict__ mu_map,
                                                            float* __restrict__ sd_map, float* __restrict__ eps_map,
                                                            float* __restrict__ out_map, int TP, int n_img,
                                                            float* __restrict__ part, unsigned* __restrict__ cnt) {
    constexpr int EPC = TT<T>::EPC;
    __shared__ float pool[DUL_RL][DUL_CV * EPC];
    __shared__ float klr[DUL_NT];
    const int t = threadIdx.x, cv = t % DUL_CV, rl = t / DUL_CV;
    const int b = blockIdx.y, cblk = blockIdx.x * DUL_CV * EPC, c0 = cblk + cv * EPC;
    float scm[EPC], shm[EPC], scl[EPC], shl[EPC], acc[EPC];
    dul_ldf<EPC>(bn_mu + c0, scm);
    dul_ldf<EPC>(bn_mu + DUL_C + c0, shm);
    dul_ldf<EPC>(bn_lv + c0, scl);
    dul_ldf<EPC>(bn_lv + DUL_C + c0, shl);
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    float kl = 0.f;
    for (int j = rl; j < TP; j += DUL_RL) {
        const size_t e0 = ((size_t)b * TP + j) * DUL_C + c0;
        float zm[EPC], zl[EPC], ep[EPC], mu[EPC], sd[EPC], o[EPC];
        dul_ldz<T>(z_mu + e0, zm);
        dul_ldz<T>(z_lv + e0, zl);
        dul_eps<EPC>(eps_in, e0, modality, step, seed_lo, seed_hi, ep);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            mu[e] = fmaf(zm[e], scm[e], shm[e]);
            sd[e] = expf(0.5f * fmaf(zl[e], scl[e], shl[e]));
            o[e] = fmaf(ep[e], sd[e], mu[e]);
            acc[e] += o[e];
            const float s2 = sd[e] * sd[e];
            kl += 0.5f * (s2 + mu[e] * mu[e] - logf(s2 + 1e-8f) - 1.f);
        }
        if (MAPS) {
            if (mu_map) dul_stf<EPC>(mu_map + e0, mu);
            if (sd_map) dul_stf<EPC>(sd_map + e0, sd);
            if (eps_map) dul_stf<EPC>(eps_map + e0, ep);
            if (out_map) dul_stf<EPC>(out_map + e0, o);
        }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) pool[rl][cv * EPC + e] = acc[e];
    klr[t] = kl;
    __syncthreads();
    if (t < DUL_CV * EPC) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < DUL_RL; ++r) s += pool[r][t];
        f[(size_t)b * DUL_C + cblk + t] = s / (float)TP;
    }
    for (int o = DUL_NT / 2; o > 0; o >>= 1) {
        if (t < o) klr[t] += klr[t + o];
        __syncthreads();
    }
    if (t < 64) {
        const int nblk = gridDim.x * gridDim.y;
        int last = 0;
        if (t == 0) {
            st_agent(part + blockIdx.y * gridDim.x + blockIdx.x, klr[0]);
            last = ticket_draw(cnt, nblk);
        }
        last = __shfl(last, 0);
        if (last) {
            const float m = ticket_fold256(part, nblk, t);
            if (t == 0) {
                reg[0] = m / (float)n_img;
                ticket_hand_back(cnt);
            }
        }
    }
}

// ---------------------------------------------------------------- backward
// d_mu, d_lv of one element (one body for the reduce and the apply pass: both see the same bits)
__device__ __forceinline__ void dul_grad1(float zm, float zl, float ep, float g, float k, float scm, float shm, float scl, float shl,
                                          float& dmu, float& dlv) {
    const float mu = fmaf(zm, scm, shm);
    const float sd = expf(0.5f * fmaf(zl, scl, shl));
    dmu = fmaf(k, mu, g);
    const float dsd = fmaf(g, ep, k * (sd - sd / fmaf(sd, sd, 1e-8f)));
    dlv = dsd * 0.5f * sd;
}

// the per-channel constants of a thread's EPC channels
template <int EPC>
struct DulChan {
    float scm[EPC], shm[EPC], mum[EPC], rsm[EPC], scl[EPC], shl[EPC], mul[EPC], rsl[EPC];
    __device__ __forceinline__ void load(const float* __restrict__ bn_mu, const float* __restrict__ bn_lv, int c0) {
        dul_ldf<EPC>(bn_mu + c0, scm);
        dul_ldf<EPC>(bn_mu + DUL_C + c0, shm);
        dul_ldf<EPC>(bn_mu + 2 * DUL_C + c0, mum);
        dul_ldf<EPC>(bn_mu + 3 * DUL_C + c0, rsm);
        dul_ldf<EPC>(bn_lv + c0, scl);
        dul_ldf<EPC>(bn_lv + DUL_C + c0, shl);
        dul_ldf<EPC>(bn_lv + 2 * DUL_C + c0, mul);
        dul_ldf<EPC>(bn_lv + 3 * DUL_C + c0, rsl);
    }
};

// pass 1: partial_mu / partial_lv [block][512][2] = { sum d, sum d xhat } of the stack, gdl_bn_bwd_finalize's format
template <typename T>
__global__ __launch_bounds__(DUL_NT) void dul_bwd_reduce_kernel(const T* __restrict__ z_mu, const T* __restrict__ z_lv,
                                                                const float* __restrict__ df, const float* __restrict__ eps_in,
                                                                uint32_t seed_lo, uint32_t seed_hi, int64_t step, int modality,
                                                                float k, const float* __restrict__ bn_mu,
                                                                const float* __restrict__ bn_lv, float* __restrict__ partial_mu,
                                                                float* __restrict__ partial_lv, size_t nvec, int TP,
                                                                size_t stride_vec) {
    constexpr int EPC = TT<T>::EPC, CPR = DUL_C / EPC, RPP = DUL_NT / CPR;
    __shared__ float red[RPP][DUL_C][4];
    size_t i = blockIdx.x * (size_t)DUL_NT + threadIdx.x;
    const int c0 = (int)(i % CPR) * EPC;  // (the stride is a multiple of CPR: a thread keeps its channels)
    DulChan<EPC> ch;
    ch.load(bn_mu, bn_lv, c0);
    float s[4][EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) s[0][e] = s[1][e] = s[2][e] = s[3][e] = 0.f;
    for (; i < nvec; i += stride_vec) {
        const size_t row = i / CPR, e0 = i * EPC;
        const int b = (int)(row / (size_t)TP);
        float zm[EPC], zl[EPC], ep[EPC], g[EPC];
        dul_ldz<T>(z_mu + e0, zm);
        dul_ldz<T>(z_lv + e0, zl);
        dul_ldf<EPC>(df + (size_t)b * DUL_C + c0, g);
        dul_eps<EPC>(eps_in, e0, modality, step, seed_lo, seed_hi, ep);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float dmu, dlv;
            dul_grad1(zm[e], zl[e], ep[e], g[e] / (float)TP, k, ch.scm[e], ch.shm[e], ch.scl[e], ch.shl[e], dmu, dlv);
            s[0][e] += dmu;
            s[1][e] += dmu * ((zm[e] - ch.mum[e]) * ch.rsm[e]);
            s[2][e] += dlv;
            s[3][e] += dlv * ((zl[e] - ch.mul[e]) * ch.rsl[e]);
        }
    }
    const int vr = threadIdx.x / CPR;
#pragma unroll
    for (int e = 0; e < EPC; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[vr][c0 + e][q] = s[q][e];
    __syncthreads();
    for (int j = threadIdx.x; j < DUL_C * 4; j += DUL_NT) {
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < RPP; ++r) a += (&red[r][0][0])[j];
        const int c = j >> 2, q = j & 3;
        st_agent((q < 2 ? partial_mu : partial_lv) + ((size_t)blockIdx.x * DUL_C + c) * 2 + (q & 1), a);
    }
}

// pass 2: dz = gamma rstd (d - coef0 - xhat coef1) of both stacks, coef[2][512] from gdl_bn_bwd_finalize
template <typename T>
__global__ __launch_bounds__(DUL_NT) void dul_bwd_apply_kernel(const T* __restrict__ z_mu, const T* __restrict__ z_lv,
                                                               const float* __restrict__ df, const float* __restrict__ eps_in,
                                                               uint32_t seed_lo, uint32_t seed_hi, int64_t step, int modality,
                                                               float k, const float* __restrict__ bn_mu,
                                                               const float* __restrict__ bn_lv, const float* __restrict__ gamma_mu,
                                                               const float* __restrict__ gamma_lv, const float* __restrict__ coef_mu,
                                                               const float* __restrict__ coef_lv, T* __restrict__ dz_mu,
                                                               T* __restrict__ dz_lv, size_t nvec, int TP, size_t stride_vec) {
    constexpr int EPC = TT<T>::EPC, CPR = DUL_C / EPC;
    size_t i = blockIdx.x * (size_t)DUL_NT + threadIdx.x;
    if (i >= nvec) return;
    const int c0 = (int)(i % CPR) * EPC;
    DulChan<EPC> ch;
    ch.load(bn_mu, bn_lv, c0);
    float grm[EPC], grl[EPC], k1m[EPC], k2m[EPC], k1l[EPC], k2l[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {  // (the BatchNorm weights are views of a parameter arena: 4-byte aligned, scalar loads)
        grm[e] = gamma_mu[c0 + e];
        grl[e] = gamma_lv[c0 + e];
    }
    dul_ldf<EPC>(coef_mu + c0, k1m);
    dul_ldf<EPC>(coef_mu + DUL_C + c0, k2m);
    dul_ldf<EPC>(coef_lv + c0, k1l);
    dul_ldf<EPC>(coef_lv + DUL_C + c0, k2l);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        grm[e] *= ch.rsm[e];
        grl[e] *= ch.rsl[e];
    }
    for (; i < nvec; i += stride_vec) {
        const size_t row = i / CPR, e0 = i * EPC;
        const int b = (int)(row / (size_t)TP);
        float zm[EPC], zl[EPC], ep[EPC], g[EPC], om[EPC], ol[EPC];
        dul_ldz<T>(z_mu + e0, zm);
        dul_ldz<T>(z_lv + e0, zl);
        dul_ldf<EPC>(df + (size_t)b * DUL_C + c0, g);
        dul_eps<EPC>(eps_in, e0, modality, step, seed_lo, seed_hi, ep);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float dmu, dlv;
            dul_grad1(zm[e], zl[e], ep[e], g[e] / (float)TP, k, ch.scm[e], ch.shm[e], ch.scl[e], ch.shl[e], dmu, dlv);
            om[e] = grm[e] * (dmu - k1m[e] - (zm[e] - ch.mum[e]) * ch.rsm[e] * k2m[e]);
            ol[e] = grl[e] * (dlv - k1l[e] - (zl[e] - ch.mul[e]) * ch.rsl[e] * k2l[e]);
        }
        *(uint4*)(dz_mu + e0) = pack16<T>(om);
        *(uint4*)(dz_lv + e0) = pack16<T>(ol);
    }
}

// ---------------------------------------------------------------- eval
// out[b][k] = fmaf(dot(W[k], f[b]) + bias[k], scale[k], shift[k]); a wave per output: lane l folds channels l, l + 64, .. l + 448
// with an fmaf chain from 0 in ascending order, then the xor butterfly 32 .. 1.  Scalar (coalesced) loads: W and bias are views
// of a parameter arena, 4-byte aligned.
__global__ __launch_bounds__(DUL_NT) void dul_eval_kernel(const float* __restrict__ f, const float* __restrict__ W,
                                                          const float* __restrict__ bias, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = f[(size_t)b * DUL_C + lane + 64 * j];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = blockIdx.x * 16 + wave * 4 + i;
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = W[(size_t)kk * DUL_C + lane + 64 * j];
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaf(w[j], x[j], a);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) out[(size_t)b * DUL_C + kk] = fmaf(a + bias[kk], scale[kk], shift[kk]);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int dul_sample_blocks(int dtype, int B) { return B * (DUL_C / (dtype == GDL_BF16 ? 8 : 4) / DUL_CV); }
// the shape checks every training entry shares
static int dul_shape(const char* who, int dtype, int n_img, int T, int P, int C, int modality) {
    GDL_REQUIRE(dtype == GDL_F32 || dtype == GDL_BF16, "%s: dtype %d", who, dtype);
    GDL_REQUIRE(C == DUL_C, "%s: built for C = 512 channels (the ResNet18 encoders' final map), got %d", who, C);
    GDL_REQUIRE(P >= 1 && T >= 1 && n_img >= 1, "%s: n_img = %d, T = %d, P = %d must all be at least 1", who, n_img, T, P);
    GDL_REQUIRE(n_img % T == 0, "%s: n_img = %d is not a multiple of T = %d", who, n_img, T);
    GDL_REQUIRE((int64_t)n_img * P < (1 << 25) && (int64_t)T * P < (1 << 24) && n_img / T <= 65535,
                "%s: n_img P = %lld rows (below 2^25), T P below 2^24, at most 65535 samples", who, (long long)n_img * P);
    GDL_REQUIRE(modality == GDL_AUDIO || modality == GDL_VISUAL, "%s: modality %d (0 audio, 1 visual)", who, modality);
    return GDL_OK;
}

}  // namespace gdl

using namespace gdl;

extern "C" {

size_t gdl_dul_sample_workspace_bytes(int dtype, int n_img, int T) {
    if ((dtype != GDL_F32 && dtype != GDL_BF16) || n_img < 1 || T < 1) return 0;
    return (64 + (size_t)dul_sample_blocks(dtype, n_img / T)) * sizeof(float);
}

int gdl_dul_sample(int dtype, const void* z_mu, const void* z_lv, const float* bn_mu, const float* bn_lv, const float* eps_in,
                   int64_t seed, int64_t step, int modality, float* f, float* reg, float* mu_map, float* sd_map, float* eps_map,
                   float* out_map, int n_img, int T, int P, int C, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = dul_shape("dul_sample", dtype, n_img, T, P, C, modality)) return rc;
    GDL_REQUIRE(z_mu && z_lv && bn_mu && bn_lv && f && reg && ws, "dul_sample: null z, bn, f, reg or workspace");
    GDL_REQUIRE(al16(z_mu) && al16(z_lv) && al16(bn_mu) && al16(bn_lv) && al16(eps_in) && al16(f) && al16(mu_map) && al16(sd_map) &&
                    al16(eps_map) && al16(out_map),
                "dul_sample: every map and per-channel array must be 16-byte aligned");
    GDL_REQUIRE(ws_bytes >= gdl_dul_sample_workspace_bytes(dtype, n_img, T) && ((uintptr_t)ws & 255) == 0,
                "dul_sample: workspace of %zu bytes, 256-byte aligned", gdl_dul_sample_workspace_bytes(dtype, n_img, T));
    const int B = n_img / T, TP = T * P;
    const bool maps = mu_map || sd_map || eps_map || out_map;
    const uint32_t slo = (uint32_t)((uint64_t)seed & 0xffffffffu), shi = (uint32_t)((uint64_t)seed >> 32);
    unsigned* cnt = (unsigned*)ws;
    float* part = (float*)ws + 64;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(dul_sample_blocks(dtype, 1), B);
    ProfScope prof("gdl::dul_sample_kernel", PROF_HBM, st, (double)n_img * P * DUL_C * (dtype == GDL_BF16 ? 4.0 : 8.0));
#define GDL_DUL_S(TY, MP)                                                                                                       \
    hipLaunchKernelGGL((dul_sample_kernel<TY, MP>), grid, dim3(DUL_NT), 0, st, (const TY*)z_mu, (const TY*)z_lv, bn_mu, bn_lv,   \
                       eps_in, slo, shi, step, modality, f, reg, mu_map, sd_map, eps_map, out_map, TP, n_img, part, cnt)
    if (dtype == GDL_BF16) {
        if (maps) GDL_DUL_S(bf16, true);
        else GDL_DUL_S(bf16, false);
    } else {
        if (maps) GDL_DUL_S(float, true);
        else GDL_DUL_S(float, false);
    }
#undef GDL_DUL_S
    GDL_CHECK_LAUNCH("dul_sample_kernel");
    return GDL_OK;
}

int gdl_dul_bwd_reduce(int dtype, const void* z_mu, const void* z_lv, const float* df, const float* eps_in, int64_t seed,
                       int64_t step, int modality, float beta, const float* bn_mu, const float* bn_lv, float* partial_mu,
                       float* partial_lv, int n_img, int T, int P, int C, void* stream) {
    if (int rc = dul_shape("dul_bwd_reduce", dtype, n_img, T, P, C, modality)) return rc;
    GDL_REQUIRE(z_mu && z_lv && df && bn_mu && bn_lv && partial_mu && partial_lv, "dul_bwd_reduce: null z, df, bn or partial");
    GDL_REQUIRE(al16(z_mu) && al16(z_lv) && al16(df) && al16(eps_in) && al16(bn_mu) && al16(bn_lv) && al16(partial_mu) &&
                    al16(partial_lv),
                "dul_bwd_reduce: every map and per-channel array must be 16-byte aligned");
    const size_t M = (size_t)n_img * P, nvec = M * DUL_C / (dtype == GDL_BF16 ? 8 : 4);
    const int blocks = bn_bwd_blocks(M, DUL_C);
    const size_t stride = (size_t)blocks * DUL_NT;
    const uint32_t slo = (uint32_t)((uint64_t)seed & 0xffffffffu), shi = (uint32_t)((uint64_t)seed >> 32);
    const float k = beta / (float)n_img;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("gdl::dul_bwd_reduce_kernel", PROF_HBM, st, (double)nvec * 16.0 * 2);
    if (dtype == GDL_BF16)
        hipLaunchKernelGGL((dul_bwd_reduce_kernel<bf16>), dim3(blocks), dim3(DUL_NT), 0, st, (const bf16*)z_mu, (const bf16*)z_lv, df,
                           eps_in, slo, shi, step, modality, k, bn_mu, bn_lv, partial_mu, partial_lv, nvec, T * P, stride);
    else
        hipLaunchKernelGGL((dul_bwd_reduce_kernel<float>), dim3(blocks), dim3(DUL_NT), 0, st, (const float*)z_mu, (const float*)z_lv,
                           df, eps_in, slo, shi, step, modality, k, bn_mu, bn_lv, partial_mu, partial_lv, nvec, T * P, stride);
    GDL_CHECK_LAUNCH("dul_bwd_reduce_kernel");
    return GDL_OK;
}

int gdl_dul_bwd_apply(int dtype, const void* z_mu, const void* z_lv, const float* df, const float* eps_in, int64_t seed,
                      int64_t step, int modality, float beta, const float* bn_mu, const float* bn_lv, const float* gamma_mu,
                      const float* gamma_lv, const float* coef_mu, const float* coef_lv, void* dz_mu, void* dz_lv, int n_img, int T,
                      int P, int C, void* stream) {
    if (int rc = dul_shape("dul_bwd_apply", dtype, n_img, T, P, C, modality)) return rc;
    GDL_REQUIRE(z_mu && z_lv && df && bn_mu && bn_lv && gamma_mu && gamma_lv && coef_mu && coef_lv && dz_mu && dz_lv,
                "dul_bwd_apply: null z, df, bn, gamma, coef or dz");
    GDL_REQUIRE(al16(z_mu) && al16(z_lv) && al16(df) && al16(eps_in) && al16(bn_mu) && al16(bn_lv) && al16(coef_mu) &&
                    al16(coef_lv) && al16(dz_mu) && al16(dz_lv),
                "dul_bwd_apply: every map, bn and coef must be 16-byte aligned (gamma: 4-byte, a parameter-arena view)");
    const size_t M = (size_t)n_img * P, nvec = M * DUL_C / (dtype == GDL_BF16 ? 8 : 4);
    size_t blocks = (nvec + DUL_NT - 1) / DUL_NT;
    if (blocks > 2048) blocks = 2048;
    const size_t stride = blocks * DUL_NT;
    const uint32_t slo = (uint32_t)((uint64_t)seed & 0xffffffffu), shi = (uint32_t)((uint64_t)seed >> 32);
    const float k = beta / (float)n_img;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("gdl::dul_bwd_apply_kernel", PROF_HBM, st, (double)nvec * 16.0 * 4);
    if (dtype == GDL_BF16)
        hipLaunchKernelGGL((dul_bwd_apply_kernel<bf16>), dim3((unsigned)blocks), dim3(DUL_NT), 0, st, (const bf16*)z_mu,
                           (const bf16*)z_lv, df, eps_in, slo, shi, step, modality, k, bn_mu, bn_lv, gamma_mu, gamma_lv, coef_mu,
                           coef_lv, (bf16*)dz_mu, (bf16*)dz_lv, nvec, T * P, stride);
    else
        hipLaunchKernelGGL((dul_bwd_apply_kernel<float>), dim3((unsigned)blocks), dim3(DUL_NT), 0, st, (const float*)z_mu,
                           (const float*)z_lv, df, eps_in, slo, shi, step, modality, k, bn_mu, bn_lv, gamma_mu, gamma_lv, coef_mu,
                           coef_lv, (float*)dz_mu, (float*)dz_lv, nvec, T * P, stride);
    GDL_CHECK_LAUNCH("dul_bwd_apply_kernel");
    return GDL_OK;
}

int gdl_dul_eval(const float* f, const float* w_mu, const float* b_mu, const float* scale, const float* shift, float* out, int B,
                 int C, void* stream) {
    GDL_REQUIRE(C == DUL_C, "dul_eval: built for C = 512 channels, got %d", C);
    GDL_REQUIRE(B >= 1 && B <= 65535, "dul_eval: B = %d samples (1 .. 65535)", B);
    GDL_REQUIRE(f && w_mu && b_mu && scale && shift && out, "dul_eval: null pointer");
    GDL_REQUIRE(f != out, "dul_eval: out must not alias f");
    GDL_REQUIRE(((uintptr_t)f & 3) == 0 && ((uintptr_t)w_mu & 3) == 0 && ((uintptr_t)out & 3) == 0, "dul_eval: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof("gdl::dul_eval_kernel", PROF_HBM, st, (double)DUL_C * DUL_C * 4.0);
    hipLaunchKernelGGL(dul_eval_kernel, dim3(DUL_C / 16, B), dim3(DUL_NT), 0, st, f, w_mu, b_mu, scale, shift, out);
    GDL_CHECK_LAUNCH("dul_eval_kernel");
    return GDL_OK;
}

}  // extern "C"
