// evalbank.hip -- the evaluation report kept on the device: what the tables this work is compared in give beyond valid()'s
// (acc, acc_a, acc_v) -- mAP, top-k and the confusion matrices of the fused / audio / visual logit sets -- from a score bank
// in ONE caller-owned device buffer, filled by one launch per batch and read with one host copy.  Not a port of a reference
// script (the reference's valid() stops at the three accuracies): it is the evaluation-side twin of the linear probe.
//
// The buffer (gdl_eval_bank_bytes(n, capacity, sets), 16-byte aligned; n <= HB_MAXN = 512, sets 1 = fused alone or 3 = fused,
// audio, visual), as eb_layout() below computes it.  All state lives in it, as the journal's does; the caller keeps the
// append offset.
//   byte 0              int64  skipped            samples whose label lies outside [0, n)
//   byte 8              int64  nonfinite[3]       per set: rows with a NaN / inf logit (of samples with a valid label)
//   byte 32             int64  num[n]             samples per class (valid labels; whatever their logits)
//   + 8 n               int64  rank_hist[sets][n] rank_hist[s][r]: samples whose label has rank r in set s; top-k = sum r < k
//   + 8 sets n          int64  confusion[sets][n][n]   row = label, column = prediction
//   ---- gdl_eval_bank_reset_bytes(n, sets) = 32 + 8 n (1 + sets + sets n): zero these bytes (hipMemsetAsync) for a new report
//   then                double ap[sets][n]        gdl_eval_bank_ap's results; NaN for a class without a positive
//   then                double mAP[3] (+ 8 bytes of padding)
//   then (16-aligned)   int32  labels[capacity]   -1 for a skipped sample (rounded up to 16 bytes)
//   then                float  probs[sets][n][capacity]   class-major: one class's scores over all samples are contiguous
// Rows at and beyond the caller's sample count are never read: labels and probs need no clearing.
//
// eval_bank_append_kernel: one 64-lane block per (sample, set); lane l holds classes l, l + 64, ... (eight at most).
//   softmax    head_body.h's spelling: mx = row maximum (exact in any order), e_j = expf(l_j - mx), se = e_0 + e_1 + ... in
//              ascending class order (one chain, walked from LDS), lse = mx + logf(se), p_j = expf(l_j - lse); stored
//              transposed, probs[s][j][row].  (head_ce_logits spreads the same sums over a 1024-thread block with the features'
//              dot products in front; its device code is left as it is.)
//   prediction first maximum, strict >, as eval_count_kernel: per lane in ascending class order, then across lanes the larger
//              value, on equal values the smaller class
//   rank       #{j : l_j > l_lab} + #{j < lab : l_j == l_lab} -- rank 0 is the event prediction == label
//   counters   64-bit integer atomics (the result does not depend on the order).  No floating-point atomic.
//   a label outside [0, n) (range-checked at 64 bits): labels[row] = -1, skipped += 1, NaN in the row's probs, nothing else
//   a non-finite logit: nonfinite[s] += 1, NaN in that set's probs of the row, no histogram / confusion entry for that set
//
// eval_bank_ap_kernel: average precision per (class, set) without a sort -- sklearn's average_precision_score on the stored
// float32 probabilities, ties grouped:  AP_c = (1 / |pos_c|) sum_{i in pos_c} #{j : label_j = c, p_jc >= p_ic} / #{j : p_jc >= p_ic},
// j over the samples with a valid label whose row of the set is finite.  One 256-thread block per (class, set), a thread per
// positive streaming the class row: the positives are found by an ordered scan of the labels (four samples a thread, ballot +
// popcount prefix, so the k-th positive in ascending sample order is the k-th entry), 256 at a time; the class row and the
// labels are staged through LDS 1024 samples at a time as keys ((bits + 1) << 1 | label == c; 0 for a sample left out), which
// every thread reads at the same address (a broadcast, eight ds_read_b128 in flight), and compared as unsigned integers: the
// probabilities are non-negative, so this is their order whatever the denormal mode.  With at most 64 positives in a pass
// (the usual case: N / n of them) the four waves hold the same positives and compare a quarter of every tile each, with at
// most 128 two pairs of waves half a tile each; the parts' integer counts are added through LDS.  Both counts are exact
// integers; the quotient is one float64 division; thread 0 adds the quotients in ascending sample order.  eval_bank_map_kernel then takes the float64 mean of the non-NaN classes in
// class order.  No block waits for another, nothing is accumulated across blocks: two calls give identical bytes.
// Cost: |pos_c| N comparisons per class, N^2 per set when every sample is kept; a class's positives beyond 256 are taken in
// further passes of the same block (one class holding all N samples is the slow case: ceil(N / 256) passes of N on one CU).
#include "common.h"
#include "head_body.h"
#include "ops.h"
#include "prof.h"

namespace gdl {

constexpr int EB_PER = HB_MAXN / 64;  // classes per lane of the append kernel
constexpr int EB_NT = 256;            // threads of the AP kernel = positives per pass
constexpr int EB_TILE = 1024;         // samples staged per LDS tile
constexpr int EB_NW = EB_NT / 64;
static_assert(EB_TILE == 4 * EB_NT && EB_NW == 4, "the AP kernel's scan and its split of a tile assume four waves and four samples a thread");
constexpr unsigned EB_INF = 0x7f800000u;

struct EbLayout {
    size_t num_at, hist_at, conf_at, reset_bytes, ap_at, map_at, labels_at, probs_at, total;
};
static EbLayout eb_layout(int n, int64_t capacity, int sets) {
    EbLayout L;
    L.num_at = 32;
    L.hist_at = L.num_at + 8 * (size_t)n;
    L.conf_at = L.hist_at + 8 * (size_t)sets * n;
    L.reset_bytes = L.conf_at + 8 * (size_t)sets * n * n;
    L.ap_at = L.reset_bytes;
    L.map_at = L.ap_at + 8 * (size_t)sets * n;
    L.labels_at = align_up(L.map_at + 32, 16);
    L.probs_at = L.labels_at + align_up(4 * (size_t)capacity, 16);
    L.total = L.probs_at + 4 * (size_t)sets * n * (size_t)capacity;
    return L;
}
static bool eb_shape_ok(int n, int64_t capacity, int sets) {
    return n >= 1 && n <= HB_MAXN && capacity >= 1 && capacity < ((int64_t)1 << 31) && (sets == 1 || sets == 3);
}

__device__ __forceinline__ bool eb_finite(float v) { return (__float_as_uint(v) & EB_INF) != EB_INF; }

__global__ __launch_bounds__(64) void eval_bank_append_kernel(unsigned char* __restrict__ bank, EbLayout L, int64_t capacity, int n,
                                                             const float* __restrict__ out, const float* __restrict__ out_a,
                                                             const float* __restrict__ out_v, const int64_t* __restrict__ labels,
                                                             int64_t offset) {
    __shared__ float ex[HB_MAXN];
    const int b = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const float* row = (s == 0 ? out : s == 1 ? out_a : out_v) + (size_t)b * n;
    const size_t r = (size_t)offset + b;
    float* probs = reinterpret_cast<float*>(bank + L.probs_at) + (size_t)s * n * (size_t)capacity + r;
    unsigned long long* skipped = reinterpret_cast<unsigned long long*>(bank);
    unsigned long long* nonfinite = reinterpret_cast<unsigned long long*>(bank + 8);
    unsigned long long* num = reinterpret_cast<unsigned long long*>(bank + L.num_at);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(bank + L.hist_at) + (size_t)s * n;
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(bank + L.conf_at) + (size_t)s * n * n;
    int* lab_out = reinterpret_cast<int*>(bank + L.labels_at);

    const long lab64 = (long)labels[b];  // range-checked at 64 bits, as eval_count_kernel does: 2^32 + k is no class k
    const bool ok = lab64 >= 0 && lab64 < n;
    const int lab = ok ? (int)lab64 : -1;
    if (s == 0 && lane == 0) {
        lab_out[r] = lab;
        atomicAdd(ok ? &num[lab] : skipped, 1ULL);
    }
    float l[EB_PER];
    bool fin = true;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < EB_PER; ++i) {
        const int j = lane + 64 * i;
        l[i] = j < n ? row[j] : -INFINITY;
        if (j < n) fin = fin && eb_finite(l[i]);
        mx = fmaxf(mx, l[i]);
    }
    const bool row_fin = __ballot(!fin) == 0ULL;
    if (!ok || !row_fin) {
        if (ok && lane == 0) atomicAdd(&nonfinite[s], 1ULL);
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < EB_PER; ++i) {
            const int j = lane + 64 * i;
            if (j < n) probs[(size_t)j * (size_t)capacity] = nan;
        }
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
#pragma unroll
    for (int i = 0; i < EB_PER; ++i) {
        const int j = lane + 64 * i;
        if (j < n) ex[j] = expf(l[i] - mx);
    }
    __syncthreads();
    float se = 0.f;
    for (int j = 0; j < n; ++j) se += ex[j];  // ascending class order; every lane walks the same chain (LDS broadcast)
    const float lse = mx + logf(se);
    // prediction and the label's rank, on the logits
    const float llab = row[lab];
    float bv = l[0];
    int bi = lane;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < EB_PER; ++i) {
        const int j = lane + 64 * i;
        if (j < n) {
            probs[(size_t)j * (size_t)capacity] = expf(l[i] - lse);
            if (l[i] > bv) {  // strict: the lane's first maximum
                bv = l[i];
                bi = j;
            }
            cnt += (l[i] > llab || (l[i] == llab && j < lab)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) {  // (lanes >= n hold -inf: a finite row never yields to them)
            bv = ov;
            bi = oi;
        }
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) {
        atomicAdd(&hist[cnt], 1ULL);
        atomicAdd(&conf[(size_t)lab * n + bi], 1ULL);
    }
}

__global__ __launch_bounds__(EB_NT) void eval_bank_ap_kernel(unsigned char* __restrict__ bank, EbLayout L, int64_t capacity, int n,
                                                            int N) {
    __shared__ __attribute__((aligned(16))) unsigned keys[EB_TILE];
    __shared__ double q[EB_NT];
    __shared__ unsigned part_all[EB_NT], part_pos[EB_NT];
    __shared__ int list[EB_NT];
    __shared__ int wcnt[EB_NW];
    const int c = blockIdx.x, s = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int* __restrict__ lab = reinterpret_cast<const int*>(bank + L.labels_at);
    const unsigned* __restrict__ row =
        reinterpret_cast<const unsigned*>(bank + L.probs_at) + ((size_t)s * n + c) * (size_t)capacity;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    double sum = 0.0;  // thread 0's
    int total = 0;
    for (int k0 = 0;; k0 += EB_NT) {
        // the positives k0 .. k0 + 255 of the class, in ascending sample order, into list[]: thread t looks at the four
        // samples base + 4 t .. + 3 of a tile, one ballot per position
        int seen = 0;
        for (int base = 0; base < N; base += EB_TILE) {
            const int j0 = base + 4 * t;
            bool f[4];
            unsigned long long mk[4];
            int before = 0, mine_cnt = 0, wave_cnt = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = j0 + u < N && lab[j0 + u] == c && row[j0 + u] <= EB_INF;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                mk[u] = __ballot(f[u]);
                before += __popcll(mk[u] & below);
                wave_cnt += __popcll(mk[u]);
            }
            if (lane == 0) wcnt[wave] = wave_cnt;
            __syncthreads();
            int off = seen - k0 + before, tile = 0;
#pragma unroll
            for (int w = 0; w < EB_NW; ++w) {
                if (w < wave) off += wcnt[w];
                tile += wcnt[w];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ord = off + mine_cnt;
                if (f[u] && ord >= 0 && ord < EB_NT) list[ord] = j0 + u;
                mine_cnt += f[u] ? 1 : 0;
            }
            seen += tile;
            __syncthreads();
        }
        total = seen;
        if (total == 0) break;  // (uniform: every thread has the same count)
        const int m = min(EB_NT, total - k0);
        // Up to 64 positives: the four waves hold the same 64 and take a quarter of every tile each; up to 128: two pairs of
        // waves, half a tile each; beyond: a wave per 64 positives, whole tiles.  The parts' counts are integers: adding them
        // is exact in any order.  A wave whose 64 positives do not exist only stages.
        const int split = m <= 64 ? 4 : m <= 128 ? 2 : 1;
        const int p = 64 * (wave / split) + lane, part = wave % split;
        const unsigned mine = p < m ? (row[list[p]] + 1u) << 1 : 0xffffffffu;
        const bool busy = 64 * (wave / split) < m;
        const int per = EB_TILE / split;  // keys of a tile this wave compares: [part per, (part + 1) per)
        unsigned n_all = 0, n_pos = 0;
        for (int base = 0; base < N; base += EB_TILE) {
#pragma unroll
            for (int u = 0; u < EB_TILE / EB_NT; ++u) {
                const int j = base + t + EB_NT * u;
                unsigned key = 0;  // left out, or beyond N: below every positive's key
                if (j < N) {
                    const unsigned bits = row[j];
                    const int lj = lab[j];
                    if (lj >= 0 && bits <= EB_INF) key = ((bits + 1u) << 1) | (lj == c ? 1u : 0u);
                }
                keys[t + EB_NT * u] = key;
            }
            __syncthreads();
            if (busy) {
                const uint4* k4 = reinterpret_cast<const uint4*>(keys + part * per);
                const int groups = (min(per, max(N - base - part * per, 0)) + 31) >> 5;  // 32 keys a group; the tail's keys are 0
                for (int g = 0; g < groups; ++g) {
                    uint4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = k4[8 * g + u];  // eight reads in flight in front of the compares
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const unsigned a0 = v[u].x >= mine, a1 = v[u].y >= mine, a2 = v[u].z >= mine, a3 = v[u].w >= mine;
                        n_all += a0 + a1 + a2 + a3;
                        n_pos += (a0 & v[u].x) + (a1 & v[u].y) + (a2 & v[u].z) + (a3 & v[u].w);
                    }
                }
            }
            __syncthreads();
        }
        part_all[t] = n_all;  // [wave][lane] = [group][part][lane]
        part_pos[t] = n_pos;
        __syncthreads();
        if (t < m) {
            const int at = 64 * split * (t >> 6) + (t & 63);
            unsigned a = 0, b = 0;
            for (int w = 0; w < split; ++w) {
                a += part_all[at + 64 * w];
                b += part_pos[at + 64 * w];
            }
            q[t] = (double)b / (double)a;  // (a >= 1: the positive itself)
        }
        __syncthreads();
        if (t == 0)
            for (int u = 0; u < m; ++u) sum += q[u];
        if (k0 + EB_NT >= total) break;  // (no further pass: the scan is not repeated to find that out)
    }
    if (t == 0) {
        double* ap = reinterpret_cast<double*>(bank + L.ap_at);
        ap[(size_t)s * n + c] = total > 0 ? sum / (double)total : __builtin_nan("");
    }
}

__global__ __launch_bounds__(64) void eval_bank_map_kernel(unsigned char* __restrict__ bank, EbLayout L, int n, int sets) {
    const int s = threadIdx.x;
    if (s >= sets) return;
    const double* ap = reinterpret_cast<const double*>(bank + L.ap_at) + (size_t)s * n;
    double sum = 0.0;
    int cnt = 0;
    for (int c = 0; c < n; ++c) {
        const double v = ap[c];
        if (v == v) {
            sum += v;
            ++cnt;
        }
    }
    reinterpret_cast<double*>(bank + L.map_at)[s] = cnt ? sum / (double)cnt : __builtin_nan("");
}

size_t eval_bank_bytes(int n, int64_t capacity, int sets) {
    return eb_shape_ok(n, capacity, sets) ? eb_layout(n, capacity, sets).total : 0;
}
size_t eval_bank_reset_bytes(int n, int sets) { return eb_shape_ok(n, 1, sets) ? eb_layout(n, 1, sets).reset_bytes : 0; }

int eval_bank_append(void* bank, int n, int64_t capacity, int sets, const float* out, const float* out_a, const float* out_v,
                     const int64_t* labels, int B, int64_t offset, hipStream_t st) {
    const EbLayout L = eb_layout(n, capacity, sets);
    ProfScope prof("gdl::eval_bank_append_kernel", PROF_HBM, st, (double)sets * B * n * 8.0);
    hipLaunchKernelGGL(eval_bank_append_kernel, dim3(B, sets), dim3(64), 0, st, (unsigned char*)bank, L, capacity, n, out, out_a,
                       out_v, labels, offset);
    GDL_CHECK_LAUNCH("eval_bank_append_kernel");
    return GDL_OK;
}

int eval_bank_ap(void* bank, int n, int64_t capacity, int sets, int64_t N, hipStream_t st) {
    const EbLayout L = eb_layout(n, capacity, sets);
    {
        ProfScope prof("gdl::eval_bank_ap_kernel", PROF_HBM, st, (double)sets * n * (double)N * 8.0);
        hipLaunchKernelGGL(eval_bank_ap_kernel, dim3(n, sets), dim3(EB_NT), 0, st, (unsigned char*)bank, L, capacity, n, (int)N);
        GDL_CHECK_LAUNCH("eval_bank_ap_kernel");
    }
    hipLaunchKernelGGL(eval_bank_map_kernel, dim3(1), dim3(64), 0, st, (unsigned char*)bank, L, n, sets);
    GDL_CHECK_LAUNCH("eval_bank_map_kernel");
    return GDL_OK;
}

}  // namespace gdl
