// philox.h -- the counter-based normal generator shared by the OGM-GE modulation (optim.hip) and the probabilistic-embedding
// branch (dul.hip): Philox4x32-10 and Box-Muller.  A value is a function of its counter and key only, never of the launch
// geometry.  The two users draw from disjoint counter ranges (word 1 of the counter, see dul_noise4).  The epoch planner of the
// device-resident loader (loader.hip) reads the raw words of the same generator with word 1 = 0xC0000000 | purpose << 24 |
// t << 8 | k: bits 31 and 30 set together, which neither the modulation (word 1 < 2^29) nor the probabilistic-embedding branch
// (0x80000000 | modality) has, so the three users stay disjoint even under one seed.
#pragma once
#include "common.h"

namespace gdl {

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k.
struct Philox4 {
    uint32_t v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// Box-Muller on a pair of words, u(w) = ((w >> 8) + 0.5) 2^-24: r = sqrt(-2 ln u(wa)), theta = 2 pi u(wb).  (w >> 8) + 0.5 has
// 25 significant bits, so the radius takes its logarithm in double: a float u rounds to 1 next to it, where ln u is all error.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float r = (float)sqrt(-2.0 * log(((double)(wa >> 8) + 0.5) * 0x1p-24));
    const float th = 6.283185307179586f * (((float)(wb >> 8) + 0.5f) * 0x1p-24f);
    float sn, cs;
    sincosf(th, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}

// The modulation's keying: the four normals of the aligned group of arena elements 4 q .. 4 q + 3 at `step`: element i takes
// z[i & 3].  Counter (q low, q high, step low, step high), key (seed low, seed high); q = i >> 2 < 2^61, so word 1 < 2^29.
__device__ __forceinline__ void noise4(int64_t q, int64_t step, uint32_t seed_lo, uint32_t seed_hi, float (&z)[4]) {
    const Philox4 w = philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)step, (uint32_t)((uint64_t)step >> 32),
                                    seed_lo, seed_hi);
    box_muller(w.v[0], w.v[1], z[0], z[1]);
    box_muller(w.v[2], w.v[3], z[2], z[3]);
}

// The probabilistic-embedding branch's keying: the four normals of elements 4 q .. 4 q + 3 of a [n_img][P][512] map (q < 2^32)
// of `modality` (0 audio, 1 visual) at `step`: counter (q, 0x80000000 | modality, step low, step high), key (seed low, seed
// high).  Word 1 has bit 31 set, which no modulation counter has, and differs between the modalities.
__device__ __forceinline__ void dul_noise4(uint32_t q, int modality, int64_t step, uint32_t seed_lo, uint32_t seed_hi, float (&z)[4]) {
    const Philox4 w = philox4x32_10(q, 0x80000000u | (uint32_t)modality, (uint32_t)step, (uint32_t)((uint64_t)step >> 32), seed_lo,
                                    seed_hi);
    box_muller(w.v[0], w.v[1], z[0], z[1]);
    box_muller(w.v[2], w.v[3], z[2], z[3]);
}

}  // namespace gdl
