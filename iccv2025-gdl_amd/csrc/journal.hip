// journal.hip -- the scripts' per-step log kept on the device: what main_dgl.py appends to its CSV at every step
// ([audio_grad_sum, visual_grad_sum], :132-152), adds into its epoch sums (`_loss += loss.item()`, :156-165), prints every 100
// steps (the losses, torch.abs(out_a).mean(), torch.abs(out_v).mean(), :125-127, :144-146), and main.py's extras (the two
// diversity sums :339-340, OGM's `ratio v / coefficient v / coefficient a` :308-312) -- as one row of GDL_JOURNAL_COLS floats
// per step in a ring, with the epoch's sums beside it, so that a whole epoch needs no host sync and one host copy.
//
// The buffer (gdl_journal_bytes(capacity), 16-byte aligned), header, then accumulators, then rows:
//   byte   0: int64  count     rows appended since the caller last zeroed the first JR_ROWS_AT bytes
//   byte   8: int64  reserved[3]
//   byte  32: double acc[12]   acc[c] = sum over all `count` rows of column c (c = 0..10), each row's float widened to double and
//                              added in step order: `s = 0.0; s += float(v)` per step, the script's own sum; acc[11] unused
//   byte 128: float  rows[capacity][16]   row `count % capacity` is written: the ring keeps the newest `capacity` rows
// Columns: 0-2 loss_f, loss_a, loss_v | 3-6 total_norm, clip_coef, audio_grad_sum, visual_grad_sum (gdl_optim_grad_stats'
// stats[0..3]) | 7-8 mean |out_a|, mean |out_v| | 9-10 a_diversity, v_diversity | 11-15 score_a, score_v, ratio_v, coeff_a,
// coeff_v (gdl_optim_modulate's mod_stats[0..4]).  All but 7-8 are copies of the source floats; a NULL source writes NaN.
//
// One launch of ONE 256-thread block.  mean |x| over n values, float32, in one fixed order: thread t adds |x[t]|, |x[t + 256]|,
// ... in turn (a chain of ceil(n / 256) terms), the xor butterfly 32 ... 1 folds a wave (six levels), the four wave sums meet
// in LDS as (w0 + w1) + (w2 + w3) (two levels), one division by (float)n.  No floating-point atomic: two launches on the same
// data give the same bits.  All terms are non-negative, so the relative error against the exact mean of the same float32
// values is at most (ceil(n / 256) + 8 + 1) 2^-24 (n < 2^24, where (float)n is exact).
// Lanes 0..15 of wave 0 then hold one column each: they store the row, lanes 0..10 add their column to acc[], lane 0 stores
// count + 1 -- ordinary stores from vector lanes.  The cursor lives in the buffer, not on the host: every step's call has the
// same arguments (it can be captured into a graph), and a new epoch is the caller's hipMemsetAsync of the first 128 bytes.
// Launches on one buffer must be ordered on one stream: the single block is the single writer.
#include "common.h"
#include "ops.h"
#include "prof.h"

namespace gdl {

constexpr int JR_NT = 256;  // threads
constexpr int JR_NW = JR_NT / 64;
constexpr int JR_COLS = GDL_JOURNAL_COLS;
constexpr int JR_NACC = 11;      // columns 0..10 have an epoch sum
constexpr int JR_ACC_AT = 32;    // byte offset of acc[]
constexpr int JR_ROWS_AT = 128;  // byte offset of rows[][]
static_assert(JR_COLS == 16 && JR_ACC_AT + (JR_NACC + 1) * 8 == JR_ROWS_AT, "journal layout");

__global__ __launch_bounds__(JR_NT) void journal_append_kernel(unsigned char* __restrict__ journal, int64_t capacity,
                                                              const float* __restrict__ losses, int n_losses,
                                                              const float* __restrict__ stats, const float* __restrict__ out_a,
                                                              const float* __restrict__ out_v, int64_t n_logits,
                                                              const float* __restrict__ div_a, const float* __restrict__ div_v,
                                                              const float* __restrict__ ogm) {
    __shared__ float wsum[2][JR_NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float sa = 0.f, sv = 0.f;
    if (out_a)
        for (int64_t i = t; i < n_logits; i += JR_NT) sa += fabsf(out_a[i]);
    if (out_v)
        for (int64_t i = t; i < n_logits; i += JR_NT) sv += fabsf(out_v[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sv += __shfl_xor(sv, o, 64);
    }
    if (lane == 0) {
        wsum[0][wave] = sa;
        wsum[1][wave] = sv;
    }
    __syncthreads();
    if (t >= JR_COLS) return;
    int64_t* count = reinterpret_cast<int64_t*>(journal);
    double* acc = reinterpret_cast<double*>(journal + JR_ACC_AT);
    const int64_t cnt = *count;
    int64_t r = cnt % capacity;
    if (r < 0) r += capacity;  // (a header the caller never zeroed: still a row of the ring, never outside it)
    float* row = reinterpret_cast<float*>(journal + JR_ROWS_AT) + r * JR_COLS;
    const float nan = __builtin_nanf("");
    float v;
    if (t < 3) {
        v = losses[n_losses == 3 ? t : 0];
    } else if (t < 7) {
        v = stats[t - 3];
    } else if (t < 9) {
        const float* w = wsum[t - 7];
        v = (t == 7 ? out_a : out_v) ? ((w[0] + w[1]) + (w[2] + w[3])) / (float)n_logits : nan;
    } else if (t < 11) {
        const float* d = t == 9 ? div_a : div_v;
        v = d ? d[0] : nan;
    } else {
        v = ogm ? ogm[t - 11] : nan;
    }
    row[t] = v;
    if (t < JR_NACC) acc[t] += (double)v;
    if (t == 0) *count = cnt + 1;
}

size_t journal_bytes(int64_t capacity) {
    return capacity < 1 ? 0 : (size_t)JR_ROWS_AT + (size_t)capacity * JR_COLS * sizeof(float);
}

int journal_append(void* journal, int64_t capacity, const float* losses, int n_losses, const float* stats, const float* out_a,
                   const float* out_v, int64_t n_logits, const float* div_a, const float* div_v, const float* ogm,
                   hipStream_t st) {
    const double bytes = (double)((out_a ? n_logits : 0) + (out_v ? n_logits : 0)) * 4.0 + JR_COLS * 8.0;
    ProfScope prof("gdl::journal_append_kernel", PROF_HBM, st, bytes);
    hipLaunchKernelGGL(journal_append_kernel, dim3(1), dim3(JR_NT), 0, st, (unsigned char*)journal, capacity, losses, n_losses,
                       stats, out_a, out_v, n_logits, div_a, div_v, ogm);
    GDL_CHECK_LAUNCH("journal_append_kernel");
    return GDL_OK;
}

}  // namespace gdl
