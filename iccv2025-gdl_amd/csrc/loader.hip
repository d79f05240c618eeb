// loader.hip -- the epoch planner of the device-resident loader (gdl.DeviceLoader): which sample stands at which position of an
// epoch, where its audio window starts, and the crop box and flip of each of its frames, as the descriptor tables that
// gdl_wave_logspec and gdl_frames_resized_crop read -- one launch for a whole epoch, nothing drawn or copied by the host.
//
// Everything is a function of (seed, epoch, sample index) through Philox4x32-10 (philox.h): key (seed low, seed high), counter
//   (c0, 0xC0000000 | purpose << 24 | t << 8 | k, epoch low, epoch high),   purpose: PERM 0, BOX 1, FLIP 2, WAVE 3.
// Word 1 has bits 31 and 30 set, which neither the modulation's counters (word 1 < 2^29) nor the probabilistic-embedding
// branch's (0x80000000 | modality) have.  The draws of a sample are keyed by its index, never by its position, so they do not
// depend on the batch size or on how the positions are dealt to ranks; only the shuffle is keyed by the position.
//
// One thread per (position, frame); a position's thread of frame 0 also writes the position's index, label and wave row.  Each
// thread evaluates the shuffle itself (a few dozen Philox calls): no thread waits for another, nothing is atomic, nothing is
// stored or sorted.  The arithmetic is stated in include/gdl_hip.h (gdl_loader_plan) and restated in tests/loader_ref.py.
// The products, sums and quotients spelled below are the arithmetic: nothing in this file is contracted into a fused
// multiply-add, so that the restatement's doubles are the device's except for exp and sqrt.
#include "common.h"
#include "ops.h"
#include "philox.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace gdl {

constexpr int LP_NT = 256;
enum { LP_PERM = 0, LP_BOX = 1, LP_FLIP = 2, LP_WAVE = 3 };

struct LpKey {
    uint32_t seed_lo, seed_hi, epoch_lo, epoch_hi;
};

__device__ __forceinline__ Philox4 lp_words(const LpKey& key, uint32_t c0, int purpose, int t, int k) {
    return philox4x32_10(c0, 0xC0000000u | ((uint32_t)purpose << 24) | ((uint32_t)t << 8) | (uint32_t)k, key.epoch_lo, key.epoch_hi,
                         key.seed_lo, key.seed_hi);
}

// u(w) = (w + 0.5) 2^-32, in (0, 1); exact in double
__device__ __forceinline__ double lp_u(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// The keyed bijection of [0, N): a balanced Feistel network on 2 * kbits bits, walked until it lands below N.  The network
// permutes [0, 4^kbits), so the walk from v < N comes back to v at the latest: it ends, after fewer than 4 passes on average.
__device__ __forceinline__ uint32_t lp_permute(const LpKey& key, uint32_t v, uint32_t N, int kbits) {
    const uint32_t mask = (1u << kbits) - 1u;
    do {
        uint32_t L = v >> kbits, R = v & mask;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const uint32_t f = lp_words(key, R, LP_PERM, 0, r).v[0] & mask;
            const uint32_t nr = L ^ f;
            L = R;
            R = nr;
        }
        v = (L << kbits) | R;
    } while (v >= N);
    return v;
}

__global__ __launch_bounds__(LP_NT) void loader_plan_kernel(const long long* __restrict__ clips, const long long* __restrict__ frames,
                                                           const long long* __restrict__ labels, uint32_t N, int T, int kbits,
                                                           LpKey key, long long first, long long count, int shuffle, int augment,
                                                           long long start_high, LoaderDraw dr, long long* __restrict__ index,
                                                           long long* __restrict__ label, long long* __restrict__ wave_desc,
                                                           long long* __restrict__ crop_desc) {
    const long long g = (long long)blockIdx.x * LP_NT + threadIdx.x;
    const long long p = g / T;
    if (p >= count) return;
    const int t = (int)(g - p * T);
    const uint32_t pos = (uint32_t)(first + p);  // < N < 2^31
    const uint32_t idx = shuffle ? lp_permute(key, pos, N, kbits) : pos;

    if (t == 0) {
        const long long* c = clips + (size_t)idx * 5;
        const uint32_t w = lp_words(key, idx, LP_WAVE, 0, 0).v[0];
        const long long start = (long long)(((unsigned long long)w * (unsigned long long)(start_high + 1)) >> 32);
        long long* wd = wave_desc + (size_t)p * 6;
        wd[0] = c[0], wd[1] = c[1], wd[2] = c[2], wd[3] = c[3], wd[4] = start, wd[5] = c[4];
        index[p] = idx;
        label[p] = labels[idx];
    }

    const long long* f = frames + ((size_t)idx * T + t) * 3;
    const long long H = f[1], W = f[2];
    long long top = 0, left = 0, bh = H, bw = W, flip = 0;
    // (a frame the stage kernel refuses anyway gets its whole frame as the box: that kernel writes the image as NaN)
    if (augment && H >= 1 && W >= 1 && H <= 65535 && W <= 65535) {
        const double area = (double)(H * W);
        bool found = false;
        for (int k = 0; k < 10 && !found; ++k) {
            const Philox4 w = lp_words(key, idx, LP_BOX, t, k);
            const double a = area * (dr.scale_lo + (dr.scale_hi - dr.scale_lo) * lp_u(w.v[0]));
            const double r = exp(dr.log_ratio_lo + (dr.log_ratio_hi - dr.log_ratio_lo) * lp_u(w.v[1]));
            const double cw = rint(sqrt(a * r)), chh = rint(sqrt(a / r));
            if (cw > 0.0 && cw <= (double)W && chh > 0.0 && chh <= (double)H) {
                bw = (long long)cw, bh = (long long)chh;
                top = (long long)(((unsigned long long)w.v[2] * (unsigned long long)(H - bh + 1)) >> 32);
                left = (long long)(((unsigned long long)w.v[3] * (unsigned long long)(W - bw + 1)) >> 32);
                found = true;
            }
        }
        if (!found) {  // the published fallback: the central crop clamped to the ratio range (a side that rounds to 0 is 1)
            const double in_ratio = (double)W / (double)H;
            if (in_ratio < dr.ratio_lo) {
                const double v = rint((double)W / dr.ratio_lo);
                bw = W, bh = v < 1.0 ? 1 : v > (double)H ? H : (long long)v;
            } else if (in_ratio > dr.ratio_hi) {
                const double v = rint((double)H * dr.ratio_hi);
                bh = H, bw = v < 1.0 ? 1 : v > (double)W ? W : (long long)v;
            }
            top = (H - bh) / 2, left = (W - bw) / 2;
        }
        flip = lp_u(lp_words(key, idx, LP_FLIP, t, 0).v[0]) < dr.p_flip ? 1 : 0;
    }
    long long* cd = crop_desc + ((size_t)p * T + t) * 8;
    cd[0] = f[0], cd[1] = H, cd[2] = W, cd[3] = top, cd[4] = left, cd[5] = bh, cd[6] = bw, cd[7] = flip;
}

int loader_plan(const long long* clips, const long long* frames, const long long* labels, long long N, int T, unsigned long long seed,
                long long epoch, long long first, long long count, int shuffle, int augment, long long start_high,
                const LoaderDraw& dr, long long* index, long long* label, long long* wave_desc, long long* crop_desc,
                hipStream_t st) {
    int bits = 0;  // bit_length(N - 1)
    for (unsigned long long m = (unsigned long long)(N - 1); m; m >>= 1) ++bits;
    const int kbits = bits < 2 ? 1 : (bits + 1) / 2;
    const LpKey key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, (uint32_t)((unsigned long long)epoch >> 32)};
    const long long threads = count * T;
    const double bytes = (double)count * ((5 + 1 + 8) * 8.0) + (double)threads * ((3 + 8) * 8.0);
    ProfScope prof("gdl::loader_plan_kernel", PROF_HBM, st, bytes);
    hipLaunchKernelGGL(loader_plan_kernel, dim3((unsigned)((threads + LP_NT - 1) / LP_NT)), dim3(LP_NT), 0, st, clips, frames, labels,
                       (uint32_t)N, T, kbits, key, first, count, shuffle, augment, start_high, dr, index, label, wave_desc,
                       crop_desc);
    GDL_CHECK_LAUNCH("loader_plan_kernel");
    return GDL_OK;
}

}  // namespace gdl
