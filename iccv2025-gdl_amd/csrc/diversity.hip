// diversity.hip -- the feature-diversity monitor of main.py (:77-89 get_feature_diversity, applied to both encoders' final
// feature maps at every step :183-184, averaged over the epoch :339-340, :356, printed as "Audio similar / Visual similar").
//
// Per image, x_p = the 512 channels at position p (P = h w positions):
//   c_p = x_p - mean_C(x_p),  s_p = sqrt(sum_C c_p^2 / (C - 1)),  R_pq = (c_p . c_q) / (s_p s_q),  d = ||R||_F / P^2
// and the result is the mean of d over the images.  With G = the Gram matrix of the centred rows, s_p^2 = G_pp / (C - 1), so
//   R_pq = (C - 1) G_pq / sqrt(G_pp G_qq)   and   d = (C - 1) sqrt(sum_pq (G_pq / sqrt(G_pp G_qq))^2) / P^2.
// A position whose channels are all equal has G_pp = 0: NaN for that image and for the mean, as the script's 0 / 0 gives.
//
// One 256-thread block per image, all arithmetic float32 whatever the storage type (a bf16 map is widened on load; the centred
// values are never rounded back):
//   1. row means (and min / max: a row of equal values is centred to exact zeros whatever the summation order would round to)
//   2. the channel axis streamed in chunks of 32: the centred chunk [P][32] goes to LDS (P = 256 whole would be 512 KB), the
//      next chunk's loads are in flight while the 16x16 tiles of G on and above the diagonal (G is symmetric: ceil(P/16)
//      (ceil(P/16) + 1) / 2 tiles, dealt round-robin to the four waves, accumulators in registers for the whole image)
//      take their 8 exact-f32 MFMAs (mfma_f32_16x16x4f32) per tile and chunk
//   3. 1 / sqrt(G_pp) from the diagonal tiles, then sum (G_pq / sqrt(G_pp G_qq))^2 over the tiles, off-diagonal tiles twice
// The mean over images: the ticket protocol of ticket.h -- d published with an agent-scope store, the block that draws the last
// ticket folds the n_img terms in ticket_fold256's order, writes mean_out[0], adds to the epoch accumulator and hands the
// counter back at zero.
#include "common.h"
#include "ops.h"
#include "prof.h"
#include "ticket.h"

namespace gdl {

constexpr int DV_C = 512;      // channels
constexpr int DV_PMAX = 256;   // positions
constexpr int DV_KC = 32;      // channels per chunk
constexpr int DV_LD = 36;      // LDS row pitch in floats (144 bytes: 16-byte aligned rows, rows 0..7 on distinct banks)
constexpr int DV_NT = 256;     // threads
constexpr int DV_NW = DV_NT / 64;
constexpr int DV_MAXTILES = (DV_PMAX / 16) * (DV_PMAX / 16 + 1) / 2;   // 136
constexpr int DV_SLOTS = (DV_MAXTILES + DV_NW - 1) / DV_NW;            // 34 tiles per wave at most
constexpr int DV_NREG = DV_PMAX * DV_KC / DV_NT;                       // 32 staged values per thread at most

struct alignas(16) DvLds {
    float x[DV_PMAX][DV_LD];  // the centred chunk, rows P .. 16 ceil(P/16) - 1 zero
    float mean[DV_PMAX];
    float inv[DV_PMAX];       // 1 / sqrt(G_pp)
    float ps[DV_NT], pmn[DV_NT], pmx[DV_NT];  // NCHW: partial row sums / minima / maxima
    float wsum[DV_NW];
    unsigned char ti[DV_MAXTILES], tj[DV_MAXTILES];
};

template <typename T>
__device__ __forceinline__ void dv_load4(const T* p, float* f);
template <>
__device__ __forceinline__ void dv_load4<float>(const float* p, float* f) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
}
template <>
__device__ __forceinline__ void dv_load4<bf16>(const bf16* p, float* f) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    f[0] = __uint_as_float(v.x << 16), f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16), f[3] = __uint_as_float(v.y & 0xffff0000u);
}

// NCHW = false: src [P][512] of T (the engine's layout);  true: src [512][P] float32 (the drop-in boundary's tensor)
template <typename T, bool NCHW>
__global__ __launch_bounds__(DV_NT) void feature_diversity_kernel(const T* __restrict__ map, int P, float* __restrict__ per_image,
                                                                 float* __restrict__ mean_out, float* __restrict__ accum,
                                                                 float* __restrict__ part, unsigned* __restrict__ cnt, int n_img) {
    __shared__ DvLds s;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int img = blockIdx.x;
    const T* __restrict__ src = map + (size_t)img * P * DV_C;
    const int nt16 = (P + 15) >> 4, ntiles = nt16 * (nt16 + 1) / 2;
    // tile list: (ti, tj), ti <= tj, row by row
    if (t < ntiles) {
        int ti = 0, rem = t, len = nt16;
        while (rem >= len) rem -= len, --len, ++ti;
        s.ti[t] = (unsigned char)ti;
        s.tj[t] = (unsigned char)(ti + rem);
    }
    for (int i = P * DV_LD + t; i < nt16 * 16 * DV_LD; i += DV_NT) (&s.x[0][0])[i] = 0.f;  // the padding rows
    // ---- 1. row means
    if constexpr (!NCHW) {
        // a wave per row, 8 consecutive channels per lane, four rows in flight
        for (int p0 = wave; p0 < P; p0 += 4 * DV_NW) {
            float f[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + DV_NW * u;
                if (p < P) {
                    dv_load4<T>(src + (size_t)p * DV_C + lane * 8, f[u]);
                    dv_load4<T>(src + (size_t)p * DV_C + lane * 8 + 4, f[u] + 4);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + DV_NW * u;
                if (p < P) {
                    float sm = ((f[u][0] + f[u][1]) + (f[u][2] + f[u][3])) + ((f[u][4] + f[u][5]) + (f[u][6] + f[u][7]));
                    float mn = fminf(fminf(fminf(f[u][0], f[u][1]), fminf(f[u][2], f[u][3])),
                                     fminf(fminf(f[u][4], f[u][5]), fminf(f[u][6], f[u][7])));
                    float mx = fmaxf(fmaxf(fmaxf(f[u][0], f[u][1]), fmaxf(f[u][2], f[u][3])),
                                     fmaxf(fmaxf(f[u][4], f[u][5]), fmaxf(f[u][6], f[u][7])));
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        sm += __shfl_xor(sm, o);
                        mn = fminf(mn, __shfl_xor(mn, o));
                        mx = fmaxf(mx, __shfl_xor(mx, o));
                    }
                    if (lane == 0) s.mean[p] = mn == mx ? mn : sm * (1.f / DV_C);
                }
            }
        }
    } else {
        // G = 256 / P threads per position (consecutive threads = consecutive positions: coalesced), channels g, g + G, ...
        const int G = DV_NT / P;
        if (t < G * P) {
            const int g = t / P, p = t - g * P;
            float a[4] = {0.f, 0.f, 0.f, 0.f}, mn = INFINITY, mx = -INFINITY;
            for (int c = g; c < DV_C; c += 4 * G)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c + u * G < DV_C) {
                        const float v = loadT<T>(src + (size_t)(c + u * G) * P + p);
                        a[u] += v;
                        mn = fminf(mn, v);
                        mx = fmaxf(mx, v);
                    }
            s.ps[t] = (a[0] + a[2]) + (a[1] + a[3]);
            s.pmn[t] = mn;
            s.pmx[t] = mx;
        }
        __syncthreads();
        if (t < P) {
            float sm = s.ps[t], mn = s.pmn[t], mx = s.pmx[t];
            for (int g = 1; g < G; ++g) {
                sm += s.ps[g * P + t];
                mn = fminf(mn, s.pmn[g * P + t]);
                mx = fmaxf(mx, s.pmx[g * P + t]);
            }
            s.mean[t] = mn == mx ? mn : sm * (1.f / DV_C);
        }
    }
    __syncthreads();
    // ---- 2. G = sum over chunks of (centred chunk) (centred chunk)^T
    // staging: NHWC -- item = (position, 4 consecutive channels), 8 P items per chunk;  NCHW -- item = (channel, position), 32 P
    const int items = NCHW ? P * DV_KC : P * (DV_KC / 4);
    const int nit = (items + DV_NT - 1) / DV_NT;  // <= 8 (NHWC), <= 32 (NCHW)
    const float rcpP = 1.f / (float)P;
    float r[DV_NREG];
    auto fetch = [&](int kc) {
        if constexpr (!NCHW) {
#pragma unroll
            for (int i = 0; i < DV_NREG / 4; ++i)
                if (i < nit) {
                    const int idx = t + DV_NT * i;
                    if (idx < items) dv_load4<T>(src + (size_t)(idx >> 3) * DV_C + kc + 4 * (idx & 7), r + 4 * i);
                }
        } else {
#pragma unroll
            for (int i = 0; i < DV_NREG; ++i)
                if (i < nit) {
                    const int idx = t + DV_NT * i;
                    if (idx < items) {
                        const int c = fdiv_small(idx, P, rcpP);
                        r[i] = loadT<T>(src + (size_t)(kc + c) * P + (idx - c * P));
                    }
                }
        }
    };
    auto stage = [&]() {
        if constexpr (!NCHW) {
#pragma unroll
            for (int i = 0; i < DV_NREG / 4; ++i)
                if (i < nit) {
                    const int idx = t + DV_NT * i;
                    if (idx < items) {
                        const int p = idx >> 3;
                        const float m = s.mean[p];
                        *reinterpret_cast<float4*>(&s.x[p][4 * (idx & 7)]) =
                            make_float4(r[4 * i] - m, r[4 * i + 1] - m, r[4 * i + 2] - m, r[4 * i + 3] - m);
                    }
                }
        } else {
#pragma unroll
            for (int i = 0; i < DV_NREG; ++i)
                if (i < nit) {
                    const int idx = t + DV_NT * i;
                    if (idx < items) {
                        const int c = fdiv_small(idx, P, rcpP), p = idx - c * P;
                        s.x[p][c] = r[i] - s.mean[p];
                    }
                }
        }
    };
    f32x4_t acc[DV_SLOTS];
#pragma unroll
    for (int k = 0; k < DV_SLOTS; ++k) acc[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;  // fragment row, k-group
    fetch(0);
    for (int kc = 0; kc < DV_C; kc += DV_KC) {
        stage();
        __syncthreads();
        if (kc + DV_KC < DV_C) fetch(kc + DV_KC);
        // a lane's 16 bytes = its operands of four MFMAs: MFMA j of a 16-channel slab contracts channels {4 g + j}, g = 0..3
#pragma unroll
        for (int k = 0; k < DV_SLOTS; ++k) {
            const int L = wave + DV_NW * k;
            if (L < ntiles) {
                const int ra = s.ti[L] * 16 + fr, rb = s.tj[L] * 16 + fr;
#pragma unroll
                for (int sl = 0; sl < DV_KC / 16; ++sl) {
                    const float4 a = *reinterpret_cast<const float4*>(&s.x[ra][sl * 16 + 4 * fg]);
                    const float4 b = *reinterpret_cast<const float4*>(&s.x[rb][sl * 16 + 4 * fg]);
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[k], 0, 0, 0);
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[k], 0, 0, 0);
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[k], 0, 0, 0);
                    acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[k], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---- 3. accumulator element e of a lane: row 4 (lane >> 4) + e, column lane & 15 of its tile
#pragma unroll
    for (int k = 0; k < DV_SLOTS; ++k) {
        const int L = wave + DV_NW * k;
        if (L < ntiles && s.ti[L] == s.tj[L]) {
            const int e = fr - 4 * fg;  // the lane's diagonal element, if it holds one
            if (e >= 0 && e < 4) {
                const float g = e == 0 ? acc[k][0] : e == 1 ? acc[k][1] : e == 2 ? acc[k][2] : acc[k][3];
                const int p = s.ti[L] * 16 + fr;
                if (p < P) s.inv[p] = g > 0.f ? 1.f / sqrtf(g) : __builtin_nanf("");  // (G_pp = 0, or NaN: NaN)
            }
        }
    }
    __syncthreads();
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < DV_SLOTS; ++k) {
        const int L = wave + DV_NW * k;
        if (L < ntiles) {
            const int ti = s.ti[L], tj = s.tj[L], q = tj * 16 + fr;
            const float iq = q < P ? s.inv[q] : 0.f, w = ti == tj ? 1.f : 2.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = ti * 16 + 4 * fg + e;
                if (p < P && q < P) {
                    const float v = acc[k][e] * s.inv[p] * iq;
                    sq += w * (v * v);
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if (lane == 0) s.wsum[wave] = sq;
    __syncthreads();
    if (wave == 0) {
        int last = 0;
        if (lane == 0) {
            const float tot = (s.wsum[0] + s.wsum[1]) + (s.wsum[2] + s.wsum[3]);
            const float d = (float)(DV_C - 1) * sqrtf(tot) / ((float)P * (float)P);
            if (per_image) per_image[img] = d;
            st_agent(part + img, d);
            last = ticket_draw(cnt, n_img);
        }
        last = __shfl(last, 0);
        if (last) {
            float m = ticket_fold256(part, n_img, lane);
            if (lane == 0) {
                m = m / (float)n_img;
                mean_out[0] = m;
                if (accum) {  // the single writer, stream-ordered: an epoch's sum and count without a host sync
                    accum[0] += m;
                    accum[1] += 1.f;
                }
                ticket_hand_back(cnt);
            }
        }
    }
}

// ws: [0] the ticket counter on a 256-byte line of its own, [64 ..) the n_img per-image terms
size_t feature_diversity_ws_bytes(int n_img) { return (64 + (size_t)(n_img > 0 ? n_img : 0)) * sizeof(float); }

int feature_diversity(const void* map, int dtype, int layout, int n_img, int P, float* per_image, float* mean_out, float* accum,
                      void* ws, hipStream_t st) {
    GDL_REQUIRE(P >= 1 && P <= DV_PMAX && n_img >= 1, "feature_diversity: 1 <= P <= %d positions, n_img >= 1", DV_PMAX);
    GDL_REQUIRE(layout == GDL_LAYOUT_NHWC || dtype == GDL_F32, "feature_diversity: the NCHW layout is float32");
    const double bytes = (double)n_img * P * DV_C * (dtype == GDL_BF16 ? 2.0 : 4.0);
    float* part = (float*)ws + 64;
    unsigned* cnt = (unsigned*)ws;
    ProfScope prof("gdl::feature_diversity_kernel", PROF_HBM, st, bytes);
    if (layout == GDL_LAYOUT_NCHW)
        hipLaunchKernelGGL((feature_diversity_kernel<float, true>), dim3(n_img), dim3(DV_NT), 0, st, (const float*)map, P, per_image,
                           mean_out, accum, part, cnt, n_img);
    else if (dtype == GDL_BF16)
        hipLaunchKernelGGL((feature_diversity_kernel<bf16, false>), dim3(n_img), dim3(DV_NT), 0, st, (const bf16*)map, P, per_image,
                           mean_out, accum, part, cnt, n_img);
    else
        hipLaunchKernelGGL((feature_diversity_kernel<float, false>), dim3(n_img), dim3(DV_NT), 0, st, (const float*)map, P, per_image,
                           mean_out, accum, part, cnt, n_img);
    GDL_CHECK_LAUNCH("feature_diversity_kernel");
    return GDL_OK;
}

}  // namespace gdl
