"""Float64 NumPy restatement of prototypical modal rebalance as DESIGN.md section 8 states it (csrc/proto.hip, gdl.prototypes,
DGLTrainer(prototypes=...)): the distances, the softmax, the scores, the losses, u = d lossp / d f, the coefficient rule and the
prototype update -- plus the float32 mirrors of the two places where the kernels' bits are the contract (the fold of the
samples' terms and the fused multiply-add of gdl_proto_apply) and the derived error bounds of gdl_proto_ce.
tests/test_pmr_cpu.py pins all of it on the CPU (against torch float64 autograd of the literal form, and against plain loops);
tests/test_pmr_gpu.py holds the kernels to it.

Error bounds of gdl_proto_ce (u = 2^-24; first order in u; T = 16 u is the relative allowance of one expf, logf or division, the
constant of tests/head_ref.py):
  D = sum_k (f_k - P_jk)^2   every term is >= 0, so relative errors do not cancel: the subtraction's rounding enters squared (2 u),
      the term then passes through at most 8 fmaf of its lane's chain and the 6 adds of the butterfly, and one more is allowed
      for the product inside the first fmaf ("three roundings per term"): |dD| <= (3 + 8 + 6) u D = 17 u D.
  d = sqrtf(D)               halves the relative error and rounds once: |dd| <= C_D u d,  C_D = 17 / 2 + 1 = 9.5;  sim = -d.
  With E = C_D u d_max (d_max the row's largest distance), a row's softmax:
  lse                        moves by at most E with its inputs; computed: the rounding of each l - max (<= u d_max, since
      0 >= l - max >= -d_max), expf (T u), the sum of n terms >= 0 (n u), logf (T u |log se|, log se <= ln n), the add max +
      log (u |lse|, |lse| <= d_max):  |dlse| <= E + 2 u d_max + (n + T + T ln n) u =: E_lse
  p_j = expf(l_j - lse)      argument error E + E_lse + u |l_j - lse|, |l_j - lse| <= d_max + ln n, then expf (T u):
      |dp_j| <= p_j (E + E_lse + u (d_max + ln n) + T u) =: p_j eps_p     -- the form 2 C_D u d_max + (n + c) u, with the three
      roundings of magnitude u d_max written out
  the terms                  |d p_label| <= p_label eps_p;   |d (lse - l_label)| <= E_lse + E + u |lse - l_label|
  q_j = ((p_j - [j == label]) / B) / d_j     absolute, because p_label - 1 may cancel: the numerator errs by p_j eps_p + u |g_j|
      (g_j = p_j - onehot), the two divisions by T u each, d_j by C_D u:
      |dq_j| <= (p_j eps_p + (1 + 2 T + C_D) u |g_j|) / (B d_j)
  u_k = sum_j q_j (P_jk - f_k)   one rounding of the difference, n fmaf:  |du_k| <= sum_j |dq_j| |P_jk - f_k| + (n + 1) u sum_j |q_j| |P_jk - f_k|
Every bound gets an absolute floor of 2^-120 (float32 results near the subnormal range keep no relative precision).
"""
import math

import numpy as np

U = 2.0 ** -24
T = 16.0
C_D = 9.5
FLOOR = 2.0 ** -120
FEAT = 512


def proto_ce(f, P, labels):
    """Everything gdl_proto_ce computes for one modality, in float64 from the given arrays.  labels outside [0, n): no one-hot
    term, a score term of 0, a NaN loss term.  Returns a dict: d, sim [B, n]; lse [B]; p, q [B, n]; term_p, term_l [B];
    score, lossp; u [B, 512]."""
    f, P = np.asarray(f, dtype=np.float64), np.asarray(P, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    B, n = f.shape[0], P.shape[0]
    diff = P[None, :, :] - f[:, None, :]                     # [B, n, 512]: P_jk - f_bk
    d = np.sqrt((diff * diff).sum(axis=2))
    sim = -d
    mx = sim.max(axis=1)
    se = np.exp(sim - mx[:, None]).sum(axis=1)
    lse = mx + np.log(se)
    p = np.exp(sim - lse[:, None])
    ok = (labels >= 0) & (labels < n)
    lc = np.where(ok, labels, 0)
    rows = np.arange(B)
    oh = np.zeros((B, n))
    oh[rows[ok], lc[ok]] = 1.0
    term_p = np.where(ok, p[rows, lc], 0.0)
    term_l = np.where(ok, lse - sim[rows, lc], np.nan)
    g = (p - oh) / B
    q = np.divide(g, d, out=np.zeros_like(g), where=d != 0)   # zero distance: q = 0 (torch's sqrt backward: NaN)
    u = np.einsum("bj,bjk->bk", q, diff)
    return dict(d=d, sim=sim, lse=lse, p=p, q=q, term_p=term_p, term_l=term_l, score=term_p.sum(), lossp=term_l.sum() / B, u=u,
                diff=diff, g=p - oh)


def proto_ce_bounds(r, B):
    """The bounds of the module docstring for a `proto_ce` result r: dict(sim [B, n], term_p, term_l [B], u [B, 512])."""
    d, p = r["d"], r["p"]
    n = d.shape[1]
    dmax = d.max(axis=1)
    E = C_D * U * dmax
    ln_n = math.log(n) if n > 1 else 0.0
    e_lse = E + 2 * U * dmax + (n + T + T * ln_n) * U
    eps_p = E + e_lse + U * (dmax + ln_n) + T * U
    ok = ~np.isnan(r["term_l"])
    b_tl = e_lse + E + U * np.abs(np.where(ok, r["term_l"], 0.0))
    dq = np.divide(p * eps_p[:, None] + (1 + 2 * T + C_D) * U * np.abs(r["g"]), B * d, out=np.zeros_like(d), where=d != 0)
    ad = np.abs(r["diff"])
    b_u = np.einsum("bj,bjk->bk", dq, ad) + (n + 1) * U * np.einsum("bj,bjk->bk", np.abs(r["q"]), ad)
    return dict(sim=C_D * U * d + FLOOR, term_p=r["term_p"] * eps_p + FLOOR, term_l=b_tl + FLOOR, u=b_u + FLOOR)


def coefficients(score_a, score_v, alpha):
    """(rho, beta, lam) in the dtype of the scores: rho = score_a / score_v; rho > 1: audio is ahead, the visual encoder is
    helped (lam = alpha); rho < 1: beta = alpha; rho == 1 or NaN: neither."""
    sa, sv = np.asarray(score_a), np.asarray(score_v)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = sa / sv
    zero = rho.dtype.type(0)
    a = rho.dtype.type(alpha)
    return rho[()], (a if rho < 1 else zero), (a if rho > 1 else zero)


def fold256(v):
    """The float32 sum of v in the kernels' order (ticket_fold256, csrc/ticket.h): 256 partial sums p[i & 255] taking i,
    i + 256, ... in turn, then the tree p[i] += p[i + o], o = 128 .. 1."""
    v = np.asarray(v, dtype=np.float32)
    p = np.zeros(256, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, len(v), 256):
            blk = v[i0:i0 + 256]
            p[:len(blk)] += blk
        o = 128
        while o:
            p[:o] = p[:o] + p[o:2 * o]
            o >>= 1
    return p[0]


def apply_stats(terms_a, terms_v, alpha):
    """stats[8] of gdl_proto_apply in float32, bit for bit: terms_m [2, B] = the samples' p[label] and loss terms."""
    ta, tv = np.asarray(terms_a, dtype=np.float32), np.asarray(terms_v, dtype=np.float32)
    B = np.float32(ta.shape[1])
    sa, sv = fold256(ta[0]), fold256(tv[0])
    rho, beta, lam = coefficients(sa, sv, np.float32(alpha))
    with np.errstate(invalid="ignore"):
        return np.array([sa, sv, rho, beta, lam, fold256(ta[1]) / B, fold256(tv[1]) / B, 0.0], dtype=np.float32)


def fmaf32(a, b, c):
    """float32 fma(a, b, c) elementwise, correctly rounded: the product of two float32 is exact in float64, the sum is taken
    with its exact error (TwoSum) and rounded to ODD in float64, which makes the final rounding to float32 the single one."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def update(P, bank, labels, momentum, first):
    """The prototype update of one bank in float64: per class the mean of its rows (added in ascending row order), then P_c =
    mean (first) or (1 - momentum) P_c + momentum mean; a class without a row keeps its prototype.  Returns (P_new float64
    [n, 512], count int64 [n], empty, out_of_range)."""
    P = np.asarray(P, dtype=np.float64).copy()
    bank, labels = np.asarray(bank, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    n = P.shape[0]
    count = np.zeros(n, dtype=np.int64)
    for c in range(n):
        rows = bank[labels == c]
        count[c] = rows.shape[0]
        if count[c]:
            mean = np.add.accumulate(rows, axis=0)[-1] / count[c]   # (accumulate: strictly in row order, no pairwise blocks)
            P[c] = mean if first else (1.0 - momentum) * P[c] + momentum * mean
    return P, count, int((count == 0).sum()), int(((labels < 0) | (labels >= n)).sum())
