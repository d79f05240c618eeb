"""A literal NumPy restatement of the score bank of csrc/evalbank.hip (gdl_eval_bank_append / gdl_eval_bank_ap), used by
tests/test_evalbank_cpu.py, tests/test_evalbank_gpu.py and tests/golden/make_golden_evalbank.py.

  softmax     float64, of the float32 logits:  mx = max_j l_j, e_j = exp(l_j - mx), se = sum_j e_j, lse = mx + log(se),
              p_j = exp(l_j - lse)
  prediction  first maximum of the logits (np.argmax);  rank = #{j : l_j > l_lab} + #{j < lab : l_j == l_lab}: integers
  counters    num[label], rank_hist[set][rank], confusion[set][label][prediction], skipped, nonfinite[set]: integers
  a label outside [0, n): stored as -1, counted in `skipped`, NaN scores, nothing else
  a row with a NaN / inf logit: counted in nonfinite[set], NaN scores, no histogram / confusion entry for that set
  AP          exact fractions.Fraction values from integer counts on GIVEN float32 probabilities (NaN = left out):
              AP_c = (1 / |pos_c|) sum_{i in pos_c} #{j : label_j = c, p_jc >= p_ic} / #{j : p_jc >= p_ic};  None without a positive
              (scikit-learn's average_precision_score, step-wise with ties grouped; it returns 0.0 and warns where this is None)

The bound beside every probability follows tests/head_ref.py's rules for softmax_ce (u = 2^-24, T = 16 per expf / logf, first
order in u, TINY = 2^-126 absolute for a result below the normal range), for the kernel's float32 evaluation of the lines above:
  d_j = l_j - mx rounds by u |d_j|, so e_j is off by (T + |d_j|) u relative (+ TINY);  the n-term sum adds n u:
      rho   = u (n + sum_j (e_j / se) (T + |d_j|)) + n TINY / se          (relative error of se)
      b_lse = rho + T u |log se| + u |lse|
  a_j = l_j - lse rounds by u |a_j| and inherits b_lse:
      b_p   = p_j (T u + b_lse + u |a_j|) + TINY
The floor TINY means a subnormal probability the device flushed to zero is no failure.  T is head_ref's and is not raised to
fit a kernel: a value outside its bound is a finding (docs/parity_log.md "score bank" records the worst measured fraction).
AP:  |pos_c| correctly rounded float64 quotients in (0, 1], summed in float64, one division: (|pos_c| + 2) 2^-53 absolute.
mAP: that, plus (n + 2) 2^-53 for the mean over at most n classes.
"""
from fractions import Fraction

import numpy as np

from head_ref import TINY, T, U, excess  # noqa: F401 (excess: for the tests)

U64 = 2.0 ** -53


def softmax_bound(logits):
    """(p, bound) float64 [N, n] of float32 logits [N, n] whose rows are all finite."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    n = l.shape[1]
    mx = l.max(axis=1, keepdims=True)
    d = l - mx
    e = np.exp(d)
    se = e.sum(axis=1, keepdims=True)
    logse = np.log(se)
    lse = mx + logse
    a = l - lse
    p = np.exp(a)
    rho = U * (n + ((e / se) * (T + np.abs(d))).sum(axis=1, keepdims=True)) + n * TINY / se
    b_lse = rho + T * U * np.abs(logse) + U * np.abs(lse)
    return p, p * (T * U + b_lse + U * np.abs(a)) + TINY


def restate(logit_sets, labels, n):
    """logit_sets: 1 or 3 float32 [N, n] arrays; labels int64 [N].  -> dict with
    labels int32 [N] (-1 skipped), skipped, nonfinite [S], num [n], rank_hist [S, n], confusion [S, n, n] (all integers),
    pred / rank int64 [S, N] (-1 where the row is left out), probs / bound float64 [S, n, N] (NaN where left out)."""
    S = len(logit_sets)
    labels = np.asarray(labels, dtype=np.int64)
    N = labels.shape[0]
    ok = (labels >= 0) & (labels < n)
    lab = np.where(ok, labels, -1).astype(np.int32)
    r = dict(labels=lab, skipped=int((~ok).sum()), nonfinite=np.zeros(S, np.int64), num=np.bincount(lab[ok], minlength=n).astype(np.int64),
             rank_hist=np.zeros((S, n), np.int64), confusion=np.zeros((S, n, n), np.int64), pred=np.full((S, N), -1, np.int64),
             rank=np.full((S, N), -1, np.int64), probs=np.full((S, n, N), np.nan), bound=np.full((S, n, N), np.nan))
    cls = np.arange(n)
    for s, lg in enumerate(logit_sets):
        lg = np.asarray(lg, dtype=np.float32)
        assert lg.shape == (N, n)
        fin = np.isfinite(lg).all(axis=1)
        r["nonfinite"][s] = int((ok & ~fin).sum())
        use = np.flatnonzero(ok & fin)
        if use.size == 0:
            continue
        p, b = softmax_bound(lg[use])
        r["probs"][s][:, use] = p.T
        r["bound"][s][:, use] = b.T
        for i in use:
            row, c = lg[i], int(lab[i])
            pred = int(np.argmax(row))  # the first maximum
            rank = int((row > row[c]).sum() + ((row == row[c]) & (cls < c)).sum())
            r["pred"][s, i], r["rank"][s, i] = pred, rank
            r["rank_hist"][s, rank] += 1
            r["confusion"][s, c, pred] += 1
    return r


def ap_exact(probs32, labels):
    """probs32: float32 [n, N] (NaN = the sample is left out of this set), labels int32 [N] (-1 skipped).
    -> ([n] Fraction or None, [n] int |pos_c|).  Comparisons are NumPy's float32 comparisons (a subnormal is not zero)."""
    probs32 = np.asarray(probs32)
    assert probs32.dtype == np.float32
    n, N = probs32.shape
    labels = np.asarray(labels)
    out, npos = [], []
    for c in range(n):
        p = probs32[c]
        valid = (labels >= 0) & ~np.isnan(p)
        pv, is_c = p[valid], labels[valid] == c
        allv, posv = np.sort(pv), np.sort(pv[is_c])
        k = int(is_c.sum())
        npos.append(k)
        if k == 0:
            out.append(None)
            continue
        n_all = allv.size - np.searchsorted(allv, pv[is_c], side="left")  # #{j : p_j >= p_i}, in ascending sample order
        n_pos = posv.size - np.searchsorted(posv, pv[is_c], side="left")
        out.append(sum((Fraction(int(a), int(b)) for a, b in zip(n_pos, n_all)), Fraction(0)) / k)
    return out, np.asarray(npos)


def ap_bound(npos):
    return (np.asarray(npos, dtype=np.float64) + 2.0) * U64


def topk(rank_hist, k):
    """[S] exact Fractions (None for a set with no counted row)"""
    return [Fraction(int(h[:k].sum()), int(h.sum())) if h.sum() else None for h in rank_hist]


# ---------------------------------------------------------------------------------------------------- inputs
SCORE_KINDS = ("random", "halves", "equal", "spread")


def make_logits(kind, N, n, seed):
    """float32 [N, n]: 'random' 3 randn; 'halves' quantised to halves (many ties); 'equal' every row the same row;
    'spread' rows spread over more than 100 (stored probabilities subnormal or zero)."""
    r = np.random.default_rng([2031, SCORE_KINDS.index(kind), N, n, seed])
    lg = 3.0 * r.standard_normal((N, n))
    if kind == "halves":
        lg = np.round(lg) / 2.0
    elif kind == "equal":
        lg = np.repeat(lg[:1], N, axis=0)
    elif kind == "spread":
        lg = lg * 20.0 + np.linspace(-60.0, 60.0, n)[None, :]
    return lg.astype(np.float32)


def make_labels(N, n, seed):
    return np.random.default_rng([2032, N, n, seed]).integers(0, n, N).astype(np.int64)
