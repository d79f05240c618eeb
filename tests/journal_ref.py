"""NumPy restatement of the step journal (csrc/journal.hip, include/gdl_hip.h "step journal"): how a row is assembled from its
sources, the float64 statement of the two mean |x| columns with the bound the kernel's summation shape gives, the epoch sums as
the reference script forms them, and what a ring of `capacity` rows retains.  Test infrastructure only."""
import math

import numpy as np

COLUMNS = ("loss_f", "loss_a", "loss_v", "total_norm", "clip_coef", "audio_grad_sum", "visual_grad_sum", "abs_out_a", "abs_out_v",
           "a_diversity", "v_diversity", "score_a", "score_v", "ratio_v", "coeff_a", "coeff_v")
N_ACC = 11          # columns 0 .. 10 are summed over the epoch
HEADER_BYTES = 128  # int64 count + 3 reserved int64, double acc[12]; float32 rows[capacity][16] follow
ACC_AT = 32
BLOCK = 256         # threads of the kernel's one block
FOLD_LEVELS = 8     # six butterfly levels in a wave of 64, two for (w0 + w1) + (w2 + w3)


def abs_mean64(x):
    """mean |x| of the float32 values `x`, in float64 (main_dgl.py:146 `torch.abs(out_a).mean()`, exactly)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return float(np.abs(x).sum() / x.size)


def abs_mean_bound(n, block=BLOCK, fold_levels=FOLD_LEVELS):
    """Relative error bound of the kernel's float32 mean |x| over n values against abs_mean64: every term is non-negative, so
    each of the additions a value passes through -- at most ceil(n / block) along its thread's chain, then `fold_levels` --
    and the one division contribute at most one rounding of relative size 2^-24 each (first order; n < 2^24)."""
    return (math.ceil(n / block) + fold_levels + 1) * 2.0 ** -24


def make_row(losses, stats, out_a=None, out_v=None, div_a=None, div_v=None, ogm=None):
    """One row as float32 [16]: losses (3 values, or 1 = that value three times), stats[0..3], mean |out_a|, mean |out_v|
    (float64 statement, rounded to float32 once), the two diversity values, ogm[0..4]; None = NaN in its columns."""
    nan = np.float32("nan")
    row = np.full(len(COLUMNS), nan, dtype=np.float32)
    losses = np.asarray(losses, dtype=np.float32).reshape(-1)
    assert losses.size in (1, 3)
    row[0:3] = losses if losses.size == 3 else losses[0]
    row[3:7] = np.asarray(stats, dtype=np.float32).reshape(-1)[:4]
    if out_a is not None:
        row[7] = np.float32(abs_mean64(out_a))
    if out_v is not None:
        row[8] = np.float32(abs_mean64(out_v))
    if div_a is not None:
        row[9] = np.float32(div_a)
    if div_v is not None:
        row[10] = np.float32(div_v)
    if ogm is not None:
        row[11:16] = np.asarray(ogm, dtype=np.float32).reshape(-1)[:5]
    return row


def seq_sum(col):
    """the script's `_loss += x.item()` over the steps: sequential, float64, from 0.0"""
    s = 0.0
    for v in col:
        s += float(v)
    return s


def acc_of(rows):
    """float64 [N_ACC]: seq_sum of columns 0 .. 10 of float32 rows [steps, 16] (every step, retained or not)"""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, len(COLUMNS))
    return np.array([seq_sum(rows[:, c]) for c in range(N_ACC)], dtype=np.float64)


def means_of(rows):
    """{name: acc / count} for columns 0 .. 10; NaN for no rows"""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, len(COLUMNS))
    n = rows.shape[0]
    return {k: (a / n if n else float("nan")) for k, a in zip(COLUMNS[:N_ACC], acc_of(rows))}


def ring_slots(count, capacity):
    """[(slot, step)] of the rows a ring of `capacity` holds after `count` appends (step i goes to slot i % capacity), oldest
    first"""
    return [(i % capacity, i) for i in range(max(0, count - capacity), count)]


def same_bits(a, b):
    """bit-equal where both are numbers; a NaN matches a NaN (its payload is not part of any statement here)"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())
