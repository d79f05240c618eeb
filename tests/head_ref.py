"""float64 NumPy restatements of the fusion heads and the cross-entropy of csrc/head.hip, each value with a DERIVED error bound,
and the shared tables of shapes, routes and mutations.  Used by tests/test_heads_cpu.py (the bounds hold for float32 in either
summation order and a subtly wrong kernel lies at least 8 bounds outside) and by tests/test_heads_gpu.py, tests/test_joint_gpu.py
and tests/test_step_gpu.py (the kernels against them).

The operations (HD = 512 features per modality)
  concat / sum DGL head   pa = x Wx^T, pv = y Wy^T;  x_out = pa + bx, y_out = pv + by, out = pa + pv + bo
                          (concat: Wx, Wy the two halves of one [n][1024] matrix, ONE bias: bx = by = bo = b; sum: bo = bx + by)
  their backward          dx = (g_x_out + [out_reaches_xy] g_out) Wx,                          dy likewise with g_y_out, Wy
                          dWx = (g_out + [uni_in_dw] g_x_out)^T x,                             dWy likewise
                          sum: dbx = sum_b g_out + [uni] sum_b g_x_out, dby likewise;  concat: db = sum_b g_out + [uni] (.. + ..)
                          (a NULL gradient is a zero)
  gated head, staged      hx = x W1^T + b1, hy = y W2^T + b2;   s(h) = 1 / (1 + exp(-h)), swish(h) = h s(h)
                          DGL:   out = (s(hx) hy) Wo^T + bo, x_out = swish(hx) Wo^T + bo, y_out = swish(hy) Wo^T + bo
                                 dhx = (g_x_out Wo) swish'(hx), dhy likewise;   swish'(h) = s (1 + h (1 - s))
                                 dWo = g_out^T (s(hx) hy) + [uni] (g_x_out^T swish(hx) + g_y_out^T swish(hy)), dbo = column sums
                          joint: (gate, value) = (hx, hy) if x_gate else (hy, hx):  out = (s(gate) value) Wo^T + bo
                                 dm = g_out Wo;  d(value) = dm s(gate);  d(gate) = dm value s (1 - s);  dWo = g_out^T (s(gate) value)
                          both:  dx = dhx W1, dy = dhy W2;  dW1 = dhx^T x, db1 = sum_b dhx;  dW2, db2 likewise
                          Each stage is restated FROM THE INPUTS IT IS GIVEN (the device's own hx / hy / dhx / dhy in the GPU
                          tests): every comparison is one sum deep.
  softmax_ce              mx = max_j l_j, se = sum_j exp(l_j - mx), lse = mx + log(se);  loss = (1/B) sum_b (lse_b - l_b[label_b]);
                          dlogits = scale (exp(l - lse) - onehot) / B.  A label outside [0, n): NaN loss term, no one-hot term.

The bounds, u = 2^-24 (float32 unit roundoff).  First order in u throughout.
  sum of products   A float32 sum of K products a_i b_i in ANY order, fused or not, plus a bias differs from the float64 value by
                    at most  (K + 4) u (sum_i |a_i| |b_i| + |bias|)   -- Higham's gamma_K; the + 4 pays for the bias add, the
                    g_out + g_u pre-add and the store.  K: 512 (x_out, y_out, hx, hy, dx of the gated head), 1024 (out of concat /
                    sum), n (dx, dy, the class sum of dh), B (dW, dW1, db1), B times the number of gradient sets added (db, dbo, dWo).
  transcendentals   __expf, expf, logf and a division each get a relative allowance of T u  (T below; the ONE constant here that
                    is not derived -- docs/parity_log.md "fusion heads" says where it comes from).  With |h| <= 8 (asserted on the
                    inputs) the argument scaling of __expf(-h), an error of |h| u, is inside T = 16.
                    s(h): exp T, the add 1, the division T:  rel. error E_s = 2 T + 2  (the add's operand error enters scaled
                    by e / (1 + e) <= 1).
  gated logits      each product term Wo s(a) c carries (E_s + 1) u relative:  (512 + 4 + E_s + 1) u (sum |terms| + |bo|)
  gated dWo         term v (g s): (K + 4 + E_s + 1) u sum |terms|
  gated dh          r = 1 + h q, q = 1 - s:  |dq| <= (E_s s + q) u,  |dr| <= (|h| (E_s s + q) + |r|) u;  with S the class sum and
                    bS = (n + 4) u sum |g| |Wo| its bound:   |d dh| <= bS s |r| + |S| s ((E_s + 2) |r| u + |dr|)
  joint dh          d(value) = dm s:  b_dm s + |dm| s (E_s + 1) u;
                    d(gate) = dm value (s q):  b_dm |value| s q + |dm| |value| (s (E_s s + q) + 3 s q + E_s s q) u
  softmax_ce        d_j = l_j - mx rounds by u |d_j|, so exp(d_j) is off by (T + |d_j|) u relative (+ TINY = 2^-126 absolute for a
                    result below the normal range, here and for exp(l - lse));  the n-term sum of the exponentials adds n u:
                      rho  = u (n + sum_j (e_j / se) (T + |d_j|)) + n TINY / se               (relative error of se)
                      b_lse = rho + T u |log se| + u |lse|
                      b_term = b_lse + u |lse - l_label|
                      b_loss = ((ceil(B / 256) + 8 + T) u sum_b |term_b| + sum_b b_term_b) / B
                        (a slot of the 256 partial sums takes ceil(B / 256) adds, the tree 8 more, the division by B T)
                      a_j = l_j - lse rounds by u |a_j| and inherits b_lse:  b_p = p_j (T u + b_lse + u |a_j|) + TINY
                      b_dlogits = |scale| / B (b_p + (2 + T) u |p_j - onehot_j|)        (the subtraction, the scale, the division)
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
T = 16.0  # the starting value of the issue; docs/parity_log.md "fusion heads" records whether a measurement replaced it
TINY = 2.0 ** -126
HD = 512
H_MAX = 8.0  # |hx|, |hy| of every gated input set stay below this (asserted in test_heads_cpu.py)


def e_s():
    return 2.0 * T + 2.0


# ---------------------------------------------------------------------------------------------------- evaluators
class Ev:
    """How sums are taken: float64 with NumPy's own sums (the reference: `exact`), or float32 with every sum an explicit chain
    in ascending (order = +1) or descending (-1) index order."""

    def __init__(self, dtype=np.float64, order=0):
        self.dtype, self.order, self.exact = dtype, order, order == 0

    def a(self, v):
        return None if v is None else np.asarray(v).astype(self.dtype)

    def c(self, A, B):
        """[M, N] = sum_k A[m, k] B[n, k]"""
        if self.exact:
            return A @ B.T
        At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
        acc = np.zeros((A.shape[0], B.shape[0]), dtype=self.dtype)
        for k in range(A.shape[1])[::self.order]:
            acc += At[k][:, None] * Bt[k][None, :]
        return acc

    def s0(self, A):
        """column sums"""
        if self.exact:
            return A.sum(axis=0)
        acc = np.zeros(A.shape[1], dtype=self.dtype)
        for k in range(A.shape[0])[::self.order]:
            acc += A[k]
        return acc

    def s1(self, A):
        """row sums"""
        return self.s0(np.ascontiguousarray(A.T))


F64 = Ev()


def F32(order):
    return Ev(np.float32, order)


def _abs_c(A, B):
    return np.abs(A) @ np.abs(B).T


def _dot(ev, A, B, bias=None, extra=0.0, drop_k=False, no_bias=False):
    """(value, bound) of sum_k A[m, k] B[n, k] + bias[n]; the bound only from the exact evaluator.  drop_k: the last k left out;
    no_bias: the bias left out (mutations)."""
    K = A.shape[1]
    if drop_k:
        A, B = A[:, :-1], B[:, :-1]
    v = ev.c(A, B)
    if bias is not None and not no_bias:
        v = v + bias
    if not ev.exact:
        return v, None
    s = _abs_c(A, B)
    if bias is not None:
        s = s + np.abs(bias)
    return v, (K + 4 + extra) * U * s


def _colsum(ev, sets, drop_last=False):
    """(value, bound) of the column sums of the given [B, n] arrays, added (None entries skipped)."""
    sets = [g for g in sets if g is not None]
    if not sets:
        return None
    B = sets[0].shape[0]
    rows = slice(0, B - 1) if drop_last else slice(None)
    v = sum(ev.s0(g[rows]) for g in sets)
    if not ev.exact:
        return v, None
    return v, (B * len(sets) + 4) * U * sum(np.abs(g[rows]).sum(axis=0) for g in sets)


def excess(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0, a NaN or a difference on a zero bound as inf)."""
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------- concat / sum heads
def lin_fwd(ev, kind, x, y, Wx, bx, Wy, by, mut=None):
    """kind 'concat' (bx is by is the one bias) or 'sum'.  -> {out, x_out, y_out: (value, bound)}"""
    x, y, Wx, bx, Wy, by = (ev.a(v) for v in (x, y, Wx, bx, Wy, by))
    f511, nb = mut == "feat511", mut == "bias"
    bo = bx + by if (kind == "sum" and mut != "bx_for_sum") else bx
    if f511:  # feature 511 of x (the last of the first modality) left out
        xo = _dot(ev, x, Wx, bx, drop_k=True)
        out = _dot(ev, np.hstack([y, x]), np.hstack([Wy, Wx]), bo, drop_k=True)
    else:
        xo = _dot(ev, x, Wx, bx, no_bias=nb)
        out = _dot(ev, np.hstack([x, y]), np.hstack([Wx, Wy]), bo, no_bias=nb)
    return dict(out=out, x_out=xo, y_out=_dot(ev, y, Wy, by, no_bias=nb))


def _add(a, b):
    if a is None:
        return b
    return a if b is None else a + b


def lin_bwd(ev, kind, x, y, Wx, Wy, gx, gy, go, out_reaches_xy, uni_in_dw, mut=None):
    """-> concat: {dx, dy, dW [n, 1024], db}, sum: {dx, dy, dWx, dbx, dWy, dby}, each (value, bound)."""
    x, y, Wx, Wy, gx, gy, go = (ev.a(v) for v in (x, y, Wx, Wy, gx, gy, go))
    if mut == "swap":
        gx, gy = gy, gx
    reach = bool(out_reaches_xy) != (mut == "reach")
    uni = bool(uni_in_dw) != (mut == "uni")
    B, n = x.shape[0], Wx.shape[0]
    z = np.zeros((B, n), dtype=ev.dtype)
    r = {}
    for name, W, gu in (("dx", Wx, gx), ("dy", Wy, gy)):
        g = _add(gu, go if reach else None)
        r[name] = _dot(ev, z if g is None else g, np.ascontiguousarray(W.T), drop_k=mut == "class")
    dW = {}
    for name, f, gu in (("dWx", x, gx), ("dWy", y, gy)):
        g = _add(go, gu if uni else None)
        dW[name] = _dot(ev, (z if g is None else g).T, f.T, drop_k=mut == "sample")
    zero = (np.zeros(n, dtype=ev.dtype), np.zeros(n) if ev.exact else None)
    ds = mut == "sample"
    if kind == "sum":
        r["dWx"], r["dWy"] = dW["dWx"], dW["dWy"]
        r["dbx"] = _colsum(ev, [go, gx if uni else None], ds) or zero
        r["dby"] = _colsum(ev, [go, gy if uni else None], ds) or zero
    else:
        r["dW"] = (np.hstack([dW["dWx"][0], dW["dWy"][0]]), np.hstack([dW["dWx"][1], dW["dWy"][1]]) if ev.exact else None)
        r["db"] = _colsum(ev, [go, gx if uni else None, gy if uni else None], ds) or zero
    return r


# ---------------------------------------------------------------------------------------------------- gated head, by stage
def _sig(ev, h):
    return 1.0 / (1.0 + np.exp(-h))  # (h has the evaluator's dtype: float32 stays float32)


def gated_hidden(ev, x, y, W1, b1, W2, b2, mut=None):
    x, y, W1, b1, W2, b2 = (ev.a(v) for v in (x, y, W1, b1, W2, b2))
    kw = dict(drop_k=mut == "feat511", no_bias=mut == "bias")
    return dict(hx=_dot(ev, x, W1, b1, **kw), hy=_dot(ev, y, W2, b2, **kw))


def gated_logits(ev, hx, hy, Wo, bo, mut=None):
    """the DGL head's three sets from given hidden vectors"""
    hx, hy, Wo, bo = (ev.a(v) for v in (hx, hy, Wo, bo))
    kw = dict(extra=e_s() + 1, drop_k=mut == "feat511", no_bias=mut == "bias")
    sx, sy = _sig(ev, hx), _sig(ev, hy)
    return dict(out=_dot(ev, sx * hy, Wo, bo, **kw), x_out=_dot(ev, sx * hx, Wo, bo, **kw), y_out=_dot(ev, sy * hy, Wo, bo, **kw))


def gated_joint_logits(ev, hx, hy, Wo, bo, x_gate, mut=None):
    hx, hy, Wo, bo = (ev.a(v) for v in (hx, hy, Wo, bo))
    gate, val = (hx, hy) if x_gate else (hy, hx)
    return dict(out=_dot(ev, _sig(ev, gate) * val, Wo, bo, extra=e_s() + 1, drop_k=mut == "feat511", no_bias=mut == "bias"))


def gated_dh(ev, hx, hy, Wo, gx, gy, mut=None):
    """dhx, dhy of the DGL head from given hx, hy and the unimodal logit gradients (None: zero)"""
    hx, hy, Wo, gx, gy = (ev.a(v) for v in (hx, hy, Wo, gx, gy))
    if mut == "swap":
        gx, gy = gy, gx
    r = {}
    for name, h, g in (("dhx", hx, gx), ("dhy", hy, gy)):
        if g is None:
            r[name] = (np.zeros_like(h), np.zeros(h.shape) if ev.exact else None)
            continue
        S, bS = _dot(ev, g, np.ascontiguousarray(Wo.T), drop_k=mut == "class")
        s = _sig(ev, h)
        q = 1.0 - s
        rr = 1.0 + h * q
        v = S * (s * h) if mut == "act" else S * s * rr  # "act": swish where swish' belongs
        if not ev.exact:
            r[name] = (v, None)
            continue
        dr = (np.abs(h) * (e_s() * s + q) + np.abs(rr)) * U
        r[name] = (v, bS * s * np.abs(rr) + np.abs(S) * s * ((e_s() + 2) * np.abs(rr) * U + dr))
    return r


def gated_joint_dh(ev, hx, hy, Wo, go, x_gate, mut=None):
    hx, hy, Wo, go = (ev.a(v) for v in (hx, hy, Wo, go))
    gate, val = (hx, hy) if x_gate else (hy, hx)
    dm, bdm = _dot(ev, go, np.ascontiguousarray(Wo.T), drop_k=mut == "class")
    s = _sig(ev, gate)
    q = 1.0 - s
    dval = dm * s
    dgate = dm * val * s if mut == "act" else dm * val * (s * q)  # "act": s where s' = s (1 - s) belongs
    if ev.exact:
        bval = bdm * s + np.abs(dm) * s * (e_s() + 1) * U
        bgate = bdm * np.abs(val) * s * q + np.abs(dm) * np.abs(val) * (s * (e_s() * s + q) + (3 + e_s()) * s * q) * U
    else:
        bval = bgate = None
    a, b = (dgate, bgate), (dval, bval)
    return dict(dhx=a, dhy=b) if x_gate else dict(dhx=b, dhy=a)


def gated_dx(ev, dhx, dhy, W1, W2, mut=None):
    dhx, dhy, W1, W2 = (ev.a(v) for v in (dhx, dhy, W1, W2))
    d = mut == "feat511"  # hidden unit 511 left out of the sum
    return dict(dx=_dot(ev, dhx, np.ascontiguousarray(W1.T), drop_k=d), dy=_dot(ev, dhy, np.ascontiguousarray(W2.T), drop_k=d))


def gated_dw1(ev, dhx, dhy, x, y, mut=None):
    dhx, dhy, x, y = (ev.a(v) for v in (dhx, dhy, x, y))
    d = mut == "sample"
    return dict(dW1=_dot(ev, dhx.T, x.T, drop_k=d), db1=_colsum(ev, [dhx], d), dW2=_dot(ev, dhy.T, y.T, drop_k=d),
                db2=_colsum(ev, [dhy], d))


def gated_dwo(ev, a, v, gx, gy, go, uni_in_dw, mut=None):
    """dWo, dbo from given hidden vectors: a the gate of `out` (hx in the DGL head), v its value (hy); the joint head passes
    (gate, value), gx = gy = None, uni_in_dw = 0."""
    a, v, gx, gy, go = (ev.a(t) for t in (a, v, gx, gy, go))
    if mut == "swap":
        gx, gy = gy, gx
    uni = bool(uni_in_dw) != (mut == "uni")
    sa = _sig(ev, a)
    parts = [(go, sa * v)] + ([(gx, sa * a), (gy, _sig(ev, v) * v)] if uni else [])
    parts = [(g, m) for g, m in parts if g is not None]
    n = next(g for g in (go, gx, gy) if g is not None).shape[1]
    B = a.shape[0]
    rows = slice(0, B - 1) if mut == "sample" else slice(None)
    val, ab = np.zeros((n, HD), dtype=ev.dtype), np.zeros((n, HD))
    for g, m in parts:
        val = val + ev.c(g[rows].T, m[rows].T)
        if ev.exact:
            ab += _abs_c(g[rows].T, m[rows].T)
    zero = (np.zeros(n, dtype=ev.dtype), np.zeros(n) if ev.exact else None)
    return dict(dWo=(val, (B * max(len(parts), 1) + 4 + e_s() + 1) * U * ab if ev.exact else None),
                dbo=_colsum(ev, [g for g, _ in parts], mut == "sample") or zero)


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
def _fold256(ev, term):
    """the loss sum as the kernel takes it: 256 slots, sample b in slot b % 256 (float32: in the evaluator's order), then the
    tree 128, 64, .., 1"""
    if ev.exact:
        return term.sum()
    B = term.shape[0]
    part = np.zeros(256, dtype=ev.dtype)
    for b in range(B)[::ev.order]:
        part[b & 255] += term[b]
    o = 128
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o >>= 1
    return part[0]


def softmax_ce(ev, logits, labels, scale, mut=None):
    """-> {loss: (value, bound), dlogits: (value, bound)}"""
    l = ev.a(logits)
    labels = np.asarray(labels, dtype=np.int64)
    B, n = l.shape
    scale = ev.dtype(scale)
    mx = l.max(axis=1, keepdims=True)
    d = l - mx
    e = np.exp(d)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        se = ev.s1(e[:, :-1] if mut == "class" else e)  # "class": the last class left out of the sum of exponentials
        logse = np.log(se)
        lse = mx[:, 0] + logse
        ok = (labels >= 0) & (labels < n)
        lc = np.where(ok, labels, 0)
        term = np.where(ok, lse - l[np.arange(B), lc], ev.dtype(np.nan))
        Bd = ev.dtype((B - 1 if B > 1 else 2) if mut == "bm1" else B)  # "bm1": B - 1 for B (B = 1: 2)
        loss = _fold256(ev, term[:-1] if mut == "sample" else term) / Bd
        a = l - lse[:, None]
        p = np.exp(a)
        oh = np.zeros((B, n), dtype=ev.dtype)
        if mut != "onehot":
            oh[np.arange(B)[ok], lc[ok]] = 1
        dl = scale * (p - oh) / Bd
    if not ev.exact or mut is not None:
        return dict(loss=(loss, None), dlogits=(dl, None))
    rho = U * (n + ((e / se[:, None]) * (T + np.abs(d))).sum(axis=1)) + n * TINY / se
    b_lse = rho + T * U * np.abs(logse) + U * np.abs(lse)
    b_term = b_lse + U * np.abs(term)
    b_loss = ((math.ceil(B / 256) + 8 + T) * U * np.abs(term).sum() + b_term.sum()) / B
    b_p = p * (T * U + b_lse[:, None] + U * np.abs(a)) + TINY
    b_dl = abs(float(scale)) / B * (b_p + (2 + T) * U * np.abs(p - oh))
    return dict(loss=(loss, b_loss), dlogits=(dl, b_dl))


# ---------------------------------------------------------------------------------------------------- shapes, routes, inputs
# concat / sum: the batch sweep at n = 6 (1; no multiple of anything; one wave of samples; the 256-sample LDS stage of
# head_bwd_w_kernel full, one over, two passes and one), the class sweep at B = 5 (below, at and above the four waves of
# head_fwd_kernel; 34; the two large heads), and both at once
LIN_SHAPES = [(B, 6) for B in (1, 5, 64, 256, 257, 513)] + [(5, n) for n in (1, 3, 4, 5, 34, 309, 512)] + [(257, 309)]
# name -> (g_x_out, g_y_out, g_out given?, out_reaches_xy, uni_in_dw, dx/dy wanted, dW/db wanted)
LIN_ROUTES = {
    "uni": (1, 1, 0, 0, 1, 1, 1),         # the unimodal losses alone, plain autograd
    "dgl": (1, 1, 1, 0, 0, 1, 1),         # the fused DGL call
    "joint": (0, 0, 1, 1, 0, 1, 1),       # one loss on the fused logits
    "undetached": (1, 1, 1, 1, 1, 1, 1),  # the un-detached ablation
    "phase2": (0, 0, 1, 0, 0, 0, 1),      # loss_f to the head's parameters only
    "only_gx": (1, 0, 0, 0, 1, 1, 1),
    "only_gy": (0, 1, 0, 0, 1, 1, 1),
    "no_dw": (1, 1, 1, 0, 0, 1, 0),
}
GATED_SHAPES = [(1, 1), (5, 3), (5, 6), (64, 34), (257, 6), (5, 309)]
# name -> (g_x_out, g_y_out, g_out given?, uni_in_dw, dx/dy wanted, dW1.. wanted, dWo/dbo wanted) of gdl_head_gated_bwd
GATED_ROUTES = {
    "phase1": (1, 1, 0, 1, 1, 1, 1),
    "phase2": (0, 0, 1, 0, 0, 0, 1),
    "dx_only": (1, 1, 0, 1, 1, 0, 0),
    "dw1_only": (1, 1, 0, 1, 0, 1, 0),
    "all_three": (1, 1, 1, 1, 1, 1, 1),
}
# (dx/dy, dW1.., dWo/dbo wanted) of gdl_head_gated_joint_bwd
GATED_JOINT_ROUTES = {"all": (1, 1, 1), "dx_only": (1, 0, 0), "dw1_only": (0, 1, 0), "dwo_only": (0, 0, 1)}
# softmax_ce: the class edges at B = 7 (thread form below 64, wave form on 16 waves to 512, on 8 to 1024, thread form beyond), the
# batch edges (the 256 loss slots) in the thread form (n = 6) and the wave form (n = 309)
CE_SHAPES = [(7, n) for n in (1, 2, 63, 64, 65, 512, 513, 1024, 1025)] + [(B, n) for n in (6, 309) for B in (1, 255, 256, 257, 600)]
CE_SCALE = 4.0               # gdl_softmax_ce's scale in the tests
CE3_SCALES = (1.0, 4.0, 0.5)  # gdl_softmax_ce3's, one per logit set



def lin_bwd_keys(kind, want_dxy, want_dw):
    """the outputs of lin_bwd a route asks for"""
    return (("dx", "dy") if want_dxy else ()) + ((("dW", "db") if kind == "concat" else ("dWx", "dbx", "dWy", "dby")) if want_dw else ())


# The mutations of a subtly wrong kernel, by restatement (test_heads_cpu.py says when each can show).  class / sample / feat511:
# the last class, the last sample, feature (or hidden unit) 511 left out of the sum that runs over it; bias: the bias left out;
# bx_for_sum: bx where bx + by belongs; swap: g_x_out and g_y_out swapped; reach / uni: out_reaches_xy / uni_in_dw flipped;
# onehot: the one-hot term dropped; bm1: B - 1 for B; act: swish where swish' belongs (joint form: s where s (1 - s) belongs).
MUTATIONS = {
    "lin_fwd": ("feat511", "bias", "bx_for_sum"),
    "lin_bwd": ("class", "sample", "swap", "reach", "uni"),
    "gated_hidden": ("feat511", "bias"),
    "gated_logits": ("feat511", "bias"),
    "gated_joint_logits": ("feat511", "bias"),
    "gated_dh": ("class", "swap", "act"),
    "gated_joint_dh": ("class", "act"),
    "gated_dx": ("feat511",),
    "gated_dw1": ("sample",),
    "gated_dwo": ("sample", "swap", "uni"),
    "softmax_ce": ("class", "sample", "onehot", "bm1"),
}


def _feat(r, B):
    """encoder features: max(randn, 0); feature 511 kept away from zero so that leaving it out can show"""
    f = np.maximum(r.standard_normal((B, HD)), 0)
    f[:, HD - 1] = np.abs(r.standard_normal(B)) + 0.5
    return f.astype(np.float32)


@functools.lru_cache(maxsize=None)
def lin_inputs(kind, B, n):
    """x, y, Wx, bx, Wy, by (concat: W [n, 1024] and b as well, Wx / Wy its halves, bx = by = b), gx, gy, go.  float32."""
    r = np.random.default_rng([2025, kind == "sum", B, n])
    d = dict(x=_feat(r, B), y=_feat(r, B))
    W = (0.05 * r.standard_normal((n, 2 * HD))).astype(np.float32)
    bx, by = ((0.1 * r.standard_normal(n)).astype(np.float32) for _ in range(2))
    if kind == "concat":
        d.update(W=W, b=bx, Wx=W[:, :HD], Wy=W[:, HD:], bx=bx, by=bx)
    else:
        d.update(Wx=np.ascontiguousarray(W[:, :HD]), Wy=np.ascontiguousarray(W[:, HD:]), bx=bx, by=by)
    for k in ("gx", "gy", "go"):
        d[k] = (r.standard_normal((B, n)) / B).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def gated_inputs(B, n):
    r = np.random.default_rng([2026, B, n])
    d = dict(x=_feat(r, B), y=_feat(r, B))
    for k, sh in (("W1", (HD, HD)), ("b1", (HD,)), ("W2", (HD, HD)), ("b2", (HD,)), ("Wo", (n, HD)), ("bo", (n,))):
        d[k] = ((0.05 if len(sh) == 2 else 0.1) * r.standard_normal(sh)).astype(np.float32)
    # hidden unit 511 kept away from zero (its biases at 1, its column of Wo at least 0.05 in size) so that leaving it out can show
    d["b1"][HD - 1] = d["b2"][HD - 1] = 1.0
    d["Wo"][:, HD - 1] += np.copysign(np.float32(0.05), d["Wo"][:, HD - 1])
    for k in ("gx", "gy", "go"):
        d[k] = (r.standard_normal((B, n)) / B).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def ce_inputs(B, n, seed=0):
    """logits 3 randn; label n - 1 in row 0 (whose logit of that class is raised by 3) and 0 in row 1; from three rows on, row 1 has equal logits and row 2 a spread of 160
    (-80 in class 0, +80 in class n - 1).  -> (logits float32, labels int64)"""
    r = np.random.default_rng([2027, B, n, seed])
    lg = (3 * r.standard_normal((B, n))).astype(np.float32)
    lab = r.integers(0, n, B).astype(np.int64)
    lab[0] = n - 1
    lg[0, n - 1] = abs(lg[0, n - 1]) + 3  # row 0 leans to its label, so that leaving the last class out shows in a batch of one
    if B >= 2:
        lab[1] = 0
    if B >= 3:
        lg[1] = np.float32(1.5)
        lg[2, 0] = -80.0
        lg[2, n - 1] = 80.0 if n > 1 else -80.0
    return lg, lab


def ce3_inputs(B, n):
    """three logit sets under one label vector (set 0 is ce_inputs(B, n)'s) -> ([l0, l1, l2], labels)"""
    lab = ce_inputs(B, n)[1]
    return [ce_inputs(B, n, k)[0] for k in range(3)], lab


def ce_cases(B, n):
    """every (logits, labels, scale) the GPU tests hand to gdl_softmax_ce / gdl_softmax_ce3 at this shape"""
    lgs, lab = ce3_inputs(B, n)
    return [(lgs[0], lab, CE_SCALE)] + [(lg, lab, sc) for lg, sc in zip(lgs, CE3_SCALES)]
