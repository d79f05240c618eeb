"""Float64 NumPy restatement of alternating unimodal training with a shared head (MLA) as DESIGN.md section 8 states it
(csrc/mla.hip, gdl.MLATrainer): the feature mean, the projector's recursive update and its normalisation, the shaping of the
head's weight gradient, the head half-step around them, the schedule helper and the entropy-weighted test-time fusion -- plus
the derived error bounds of the four gdl_mla_* launches.  tests/test_mla_cpu.py pins all of it on the CPU (against torch
float64 autograd of the literal form and against the torch float32 goldens); tests/test_mla_gpu.py holds the kernels to it.

Error bounds (u = 2^-24; first order in u; gamma_n = n u / (1 - n u); T = 16 u is the relative allowance of one division,
expf or logf, the constant of tests/pmr_ref.py and tests/head_ref.py).  Inputs are the float32 arrays the kernel reads, taken
as exact unless a perturbation (dP, dr) is handed in, which is then propagated to first order beside the roundings:
  mean      r = (sum_b h[b]) / B: B - 1 adds and one division: |dr| <= gamma_B mean_b |h[b]| + T |r|
  k_i       = sum_j P_ij r_j, 512 terms, any order:        bk_i = gamma_512 sum_j |P_ij r_j| + sum_j (dP_ij |r_j| + |P_ij| dr_j)
  c         = alpha + r . k:     bc = sum_i |r_i| bk_i + sum_i dr_i |k_i| + gamma_512 sum_i |r_i k_i| + u |c|
  q_ij      = (k_i k_j) / c:     bq_ij = (|k_j| bk_i + |k_i| bk_j) / c + |k_i k_j| bc / c^2 + (u + T) |q_ij|
  P1_ij     = P_ij - q_ij:       bP1_ij = dP_ij + bq_ij + u |P1_ij|
  S         = sum_ij P1_ij^2, rows by 8 fmaf + 6 tree adds in float32 (every term >= 0: at most gamma_16 S), the 512 row sums in
              double (below u):  |dS| / S <= 2 sum |P1| bP1 / S + gamma_16 + u
  ||P||_F   = sqrt(S) rounded to float32:                  rel_n = |dS| / (2 S) + 2 u
  P2_ij     = P1_ij / ||P||_F:   bP2_ij = bP1_ij / ||P||_F + |P2_ij| (rel_n + T)
  project   out[c][i] = sum_j dW[c][j] P[i][j], 512 terms: gamma_512 (|dW| |P|^T)_ci  (+ |dW| dP^T when dP is given)
  fuse, per row and set, d_j = l_j - max, t_j = lse - l_j, A = sum_j p_j |d_j|:
    se      = sum_j expf(d_j): the difference's rounding moves the argument by u |d_j|, expf adds T, the ascending sum gamma_n:
              rel_se = gamma_n + T + u A
    lse     = max + logf(se):    b_lse = u |lse| + T |log se| + rel_se
    p_j     = expf(l_j - lse):   rel_p_j = T + b_lse + u t_j
    e       = sum_j p_j t_j:     b_e = gamma_n e + sum_j p_j (t_j (rel_p_j + u) + b_lse + u t_j)
    lam_a   = sigmoid(e_v - e_a) in exact arithmetic (the min only guards the exponentials), d lam / d e = lam_a lam_v:
              b_lam_m = lam_a lam_v (b_ea + b_ev + u |e_a - e_v|) + lam_m (2 T + 2 u)
    out_j   = lam_a a_j + lam_v v_j:   |a_j| b_lam_a + |v_j| b_lam_v + 2 u (|lam_a a_j| + |lam_v v_j|)
Every bound gets the absolute floor of tests/pmr_ref.py, 2^-120.
"""
import numpy as np

U = 2.0 ** -24
T = 16.0 * U
FLOOR = 2.0 ** -120
FEAT = 512


def gamma(n):
    return n * U / (1.0 - n * U)


def mla_alpha(step_in_epoch, steps_per_epoch):
    """gdl.mla_alpha restated"""
    return 0.1 ** (1.0 + step_in_epoch / steps_per_epoch)


# ------------------------------------------------------------------ the feature mean
def feature_mean(h):
    h = np.asarray(h, dtype=np.float64)
    return np.add.accumulate(h, axis=0)[-1] / h.shape[0]


def feature_mean_bound(h):
    h = np.asarray(h, dtype=np.float64)
    B = h.shape[0]
    return gamma(B) * np.abs(h).sum(axis=0) / B + T * np.abs(feature_mean(h)) + FLOOR


# ------------------------------------------------------------------ the projector
def projector_update(P, r, alpha, normalize=True):
    """One update in float64 from the given arrays; alpha is taken at float32 (it is a float kernel argument).  Returns a dict:
    k [512], c, q, P1 (before the normalisation) [512, 512], norm (||P1||_F), P (the result)."""
    P, r = np.asarray(P, dtype=np.float64), np.asarray(r, dtype=np.float64)
    a = float(np.float32(alpha))
    k = P @ r
    c = a + r @ k
    q = np.outer(k, k) / c
    P1 = P - q
    nrm = float(np.sqrt((P1 * P1).sum()))
    return dict(k=k, c=c, q=q, P1=P1, norm=nrm, P=P1 / nrm if normalize else P1, P0=P, r=r, normalize=bool(normalize))


def projector_bounds(res, dP=None, dr=None):
    """The module docstring's bounds for a `projector_update` result: dict(k, c, P) -- P's bound is that of P2 or P1 as the
    result was normalised or not.  dP [512, 512] / dr [512]: elementwise bounds on a perturbation of the inputs."""
    P0, r, k, c = np.abs(res["P0"]), np.abs(res["r"]), np.abs(res["k"]), res["c"]
    dP = np.zeros_like(P0) if dP is None else np.asarray(dP, dtype=np.float64)
    dr = np.zeros_like(r) if dr is None else np.asarray(dr, dtype=np.float64)
    g = gamma(FEAT)
    bk = g * (P0 @ r) + dP @ r + P0 @ dr
    bc = r @ bk + dr @ k + g * (r @ k) + U * abs(c)
    bq = (np.outer(bk, k) + np.outer(k, bk)) / c + np.outer(k, k) * bc / (c * c) + (U + T) * np.abs(res["q"])
    bP1 = dP + bq + U * np.abs(res["P1"])
    if not res["normalize"]:
        return dict(k=bk + FLOOR, c=bc + FLOOR, P=bP1 + FLOOR)
    S = res["norm"] ** 2
    rel_n = (2.0 * (np.abs(res["P1"]) * bP1).sum() / S + gamma(16) + U) / 2.0 + 2 * U
    bP2 = bP1 / res["norm"] + np.abs(res["P"]) * (rel_n + T)
    return dict(k=bk + FLOOR, c=bc + FLOOR, P=bP2 + FLOOR, norm=res["norm"] * rel_n + FLOOR)


def project(dW, P):
    return np.asarray(dW, dtype=np.float64) @ np.asarray(P, dtype=np.float64).T


def project_bound(dW, P, dP=None, ddW=None):
    aW, aP = np.abs(np.asarray(dW, dtype=np.float64)), np.abs(np.asarray(P, dtype=np.float64))
    b = gamma(FEAT) * (aW @ aP.T)
    if dP is not None:
        b = b + aW @ np.asarray(dP, dtype=np.float64).T
    if ddW is not None:
        b = b + np.asarray(ddW, dtype=np.float64) @ aP.T
    return b + FLOOR


def p_summary(P):
    """What the goldens keep of P (it is too large to commit whole)"""
    P = np.asarray(P)
    P64 = P.astype(np.float64)
    return dict(P16=P[:16, :16].copy(), Pdiag=np.diag(P).copy(), Prowsum=P64.sum(axis=1), Pfro=np.float64(np.sqrt((P64 * P64).sum())))


# ------------------------------------------------------------------ the head half-step
def half_step_head(h, W, b, label, P=None, r_prev=None, alpha=None, normalize=True):
    """Steps 1, 3 and 4 of a half-step in float64: logits, loss, dlogits, df, dW, db; with P and r_prev given (shaping on and a
    previous feature mean present) the projector update and dW <- dW P^T; the feature mean.  Returns a dict."""
    h, W, b = (np.asarray(x, dtype=np.float64) for x in (h, W, b))
    label = np.asarray(label, dtype=np.int64)
    B, n = h.shape[0], W.shape[0]
    out = h @ W.T + b
    mx = out.max(axis=1)
    lse = mx + np.log(np.exp(out - mx[:, None]).sum(axis=1))
    p = np.exp(out - lse[:, None])
    oh = np.zeros((B, n))
    oh[np.arange(B), label] = 1.0
    loss = (lse - out[np.arange(B), label]).sum() / B
    dl = (p - oh) / B
    res = dict(out=out, loss=loss, dlogits=dl, df=dl @ W, dW_plain=dl.T @ h, db=dl.sum(axis=0), r=feature_mean(h))
    res["dW"] = res["dW_plain"]
    if P is not None and r_prev is not None:
        res["proj"] = projector_update(P, r_prev, alpha, normalize)
        res["dW"] = project(res["dW_plain"], res["proj"]["P"])
    return res


# ------------------------------------------------------------------ the test-time fusion
def _row_stats(l):
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = l.max(axis=1)
        d = l - mx[:, None]
        se = np.exp(d).sum(axis=1)
        lse = mx + np.log(se)
        t = lse[:, None] - l
        p = np.exp(-t)
        e = np.where(p > 0, p * t, 0.0).sum(axis=1)
    return dict(l=l, mx=mx, d=d, se=se, lse=lse, t=t, p=p, e=e)


def fuse(out_a, out_v, dynamic=True):
    """(out, lam [B, 2], the two sets' row statistics) in float64.  A row with a non-finite logit in either set: NaN lam and a
    NaN out row when dynamic; with dynamic=False lam = 0.5, 0.5 and out = 0.5 out_a + 0.5 out_v whatever the logits."""
    sa, sv = _row_stats(out_a), _row_stats(out_v)
    B = sa["l"].shape[0]
    if not dynamic:
        lam = np.full((B, 2), 0.5)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            mn = np.minimum(sa["e"], sv["e"])
            wa, wv = np.exp(-(sa["e"] - mn)), np.exp(-(sv["e"] - mn))
            lam = np.stack([wa / (wa + wv), wv / (wa + wv)], axis=1)
        bad = ~(np.isfinite(sa["l"]).all(axis=1) & np.isfinite(sv["l"]).all(axis=1))
        lam[bad] = np.nan
    with np.errstate(invalid="ignore"):
        out = lam[:, :1] * sa["l"] + lam[:, 1:] * sv["l"]
    return out, lam, sa, sv


def _entropy_bound(s):
    n = s["l"].shape[1]
    A = (s["p"] * np.abs(s["d"])).sum(axis=1)
    rel_se = gamma(n) + T + U * A
    b_lse = U * np.abs(s["lse"]) + T * np.abs(np.log(s["se"])) + rel_se
    rel_p = T + b_lse[:, None] + U * s["t"]
    return gamma(n) * s["e"] + (s["p"] * (s["t"] * (rel_p + U) + b_lse[:, None] + U * s["t"])).sum(axis=1)


def fuse_bounds(out_a, out_v, dynamic=True):
    """dict(lam [B, 2], out [B, n]) for the finite rows (the others: NaN)"""
    out, lam, sa, sv = fuse(out_a, out_v, dynamic)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if dynamic:
            spread = lam[:, 0] * lam[:, 1] * (_entropy_bound(sa) + _entropy_bound(sv) + U * np.abs(sa["e"] - sv["e"]))
            b_lam = spread[:, None] + lam * (2 * T + 2 * U)
        else:
            b_lam = np.zeros_like(lam)
        la, lv = np.abs(lam[:, :1] * sa["l"]), np.abs(lam[:, 1:] * sv["l"])
        b_out = np.abs(sa["l"]) * b_lam[:, :1] + np.abs(sv["l"]) * b_lam[:, 1:] + 2 * U * (la + lv)
    return dict(lam=b_lam + FLOOR, out=b_out + FLOOR)


def replay_projector(rs, alphas, drs=None, any_order_norm=False, normalize=True):
    """The projector after the shaped half-steps of a run, from the identity: rs[i] = the feature mean update i went against,
    alphas[i] its alpha_s.  Returns (P float64, dP) with dP the bound carried through the updates by `projector_bounds`: the
    roundings of a float32 run plus, with drs[i] given, a perturbation of rs[i] of that size.  any_order_norm: the Frobenius sum
    taken in an unknown order (a torch float32 loop), gamma over all 512 x 512 terms instead of this library's gamma_16."""
    P, dP = np.eye(FEAT), np.zeros((FEAT, FEAT))
    for i, (r, a) in enumerate(zip(rs, alphas)):
        res = projector_update(P, r, a, normalize)
        dP = projector_bounds(res, dP=dP, dr=None if drs is None else drs[i])["P"]
        if any_order_norm and normalize:
            dP = dP + np.abs(res["P"]) * gamma(FEAT * FEAT) / 2
        P = res["P"]
    return P, dP
