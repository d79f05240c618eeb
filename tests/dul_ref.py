"""float64 NumPy restatement of the probabilistic-embedding branch (main.py --pe 1 --beta b) as csrc/dul.hip and gdl/dul.py
compute it: the two Conv2d(1x1) + BatchNorm2d stacks behind an encoder's final map, the reparameterised sample, its pool, the
KL term `regurize`, the backward through both BatchNorms, the pooled eval form, and the noise generator with its keying.  The
yardstick of tests/test_dul_gpu.py, itself pinned by tests/test_dul_cpu.py against torch float64 autograd of the literal form.
No GPU, no reference import.

Layout: maps are [M][512] with M = n_img P rows, row r of image r // P and of sample r // (T P).

Error bounds (the `*_bound` functions; u = 2^-24, the float32 unit roundoff; 2^-9 where a value is stored as bfloat16)
-----------------------------------------------------------------------------------------------------------------------------
The device works in float32 on the same inputs this file is given (z as stored, the float32 scale / shift / mean / rstd, the
device's own eps), so a bound has to cover the kernel's float32 roundings alone.  They are first-order forward error analyses,
every one multiplied by SAFETY = 2 for the second-order terms; none is fitted to an observed error.
  * one rounding of an exact result r costs u |r| (an fma is one rounding);
  * expf / logf / the division are taken as accurate to 2 ulp, LIBM = 4 u relative (the device library documents 1 ulp);
  * a sum whose terms each pass through at most D additions has error at most D u sum |terms|; D is read off the kernel's
    stated order: pool D = ceil(TP / 16) + 16; KL D = 8 ceil(TP / 16) + 8 + ceil(blocks / 256) + 8; the backward's channel
    sums D = (rows one thread adds in sequence) + 4 + 1 with the float32 per-block partials then added in double; the eval dot product
    D = 8 + 6.
  mu = fma(z, sc, sh)                          e_mu  = u |mu|
  sd = expf(0.5 fma(z, sc, sh))                r_sd  = LIBM + 0.5 u |lv|              (relative; 0.5 lv is exact)
  out = fma(eps, sd, mu)                       e_out = |eps| sd r_sd + e_mu + u |out|
  f = (sum out) / TP                           e_f   = (sum e_out + D u sum |out|) / TP + u |f|
  t = 0.5 (s2 + mu^2 - logf(s2 + 1e-8) - 1)    e_t   = 0.5 [ (2 r_sd + u) s2 + 3 u mu^2 + (2 r_sd + 2 u) + LIBM |log a|
                                                             + 3 u (s2 + mu^2 + |log a| + 1) ]
  reg = (sum t) / n_img                        e_reg = (sum e_t + D u sum |t|) / n_img + u |reg|
  g = df / TP, k = beta / n_img                u |g|; 2 u |k| (beta's conversion to float32 and the division)
  d_mu = fma(k, mu, g)                         e_dmu = u |g| + |k| (e_mu + 2 u |mu|) + u |d_mu|
  w = sd - sd / fma(sd, sd, 1e-8)              e_w   = sd r_sd + q (3 r_sd + 2 u + LIBM) + u |w|,  q = sd / (s2 + 1e-8)
  d_sd = fma(g, eps, k w)                      e_dsd = |eps| u |g| + |k| (e_w + 3 u |w|) + u |d_sd|
  d_lv = d_sd 0.5 sd                           e_dlv = 0.5 sd e_dsd + |d_lv| (r_sd + 2 u)
  xhat = (z - mean) rstd                       e_xh  = 2 u |xhat|
  S1 = sum d, S2 = sum d xhat                  e_S   = sum term errors + D u sum |terms| + u |S|
  coef = S / M                                 e_S / M + u |coef|
  dz = (gamma rstd) (d - c0 - xhat c1)         e_dz  = |gr| [e_d + e_c0 + |xhat| e_c1 + |c1| e_xh + 3 u (|d| + |c0| + |xhat c1|)]
                                                       + 2 u |dz|
  stored as bfloat16 (8 significant bits)      half an ulp is 2^-9 of the top of the value's binade, at most 2 * 2^-9 of the value
                                               itself: + 2 * 2^-9 (|dz| + e_dz), outside SAFETY (it is exact, not first-order)
  eval: o = fma(dot + b, sc, sh)               e_o   = |sc| (D u sum |w f| + u |dot + b|) + u |o|
"""
import numpy as np

import modulation_ref as mr

U = 2.0 ** -24
U_BF16 = 2.0 ** -9
LIBM = 4 * U
SAFETY = 2.0
C = 512
BN_EPS = 1e-5
MOMENTUM = 0.1
KL_EPS = float(np.float32(1e-8))
AUDIO, VISUAL = 0, 1


# ---------------------------------------------------------------------------------------------------------------- noise
def normals(n_elems, seed, step, modality):
    """The standard normals of elements 0 .. n_elems - 1 of a [n_img][P][512] map: counter (e >> 2, 0x80000000 | modality,
    step low, step high), key (seed low, seed high); words (0, 1) give z0, z1, words (2, 3) give z2, z3; element e takes
    z[e & 3].  Word 1 of a modulation counter (modulation_ref.normals) is index >> 34 < 2^29: the ranges are disjoint."""
    e = np.arange(n_elems, dtype=np.int64)
    q = e >> 2
    w = mr.philox4x32_10((q & mr.MASK, np.full_like(q, 0x80000000 | modality), np.full_like(q, step & mr.MASK),
                          np.full_like(q, (step >> 32) & mr.MASK)), (seed & mr.MASK, (seed >> 32) & mr.MASK))
    z = np.stack(mr.box_muller(w[0], w[1]) + mr.box_muller(w[2], w[3]))
    return np.take_along_axis(z, (e & 3)[None], axis=0)[0]


# ---------------------------------------------------------------------------------------------------------------- forward
def conv_bn_train(x, W, b, gamma, beta):
    """z = x W^T + b over the M rows and the train-mode BatchNorm constants of it: (z, scale, shift, mean, rstd, var)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64).reshape(C, C)
    z = x @ W.T + np.asarray(b, np.float64)
    mean, var = z.mean(0), z.var(0)  # biased
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    scale = np.asarray(gamma, np.float64) * rstd
    return z, scale, np.asarray(beta, np.float64) - mean * scale, mean, rstd, var


def running_update(rm, rv, mean, var, M):
    """nn.BatchNorm2d's running statistics after one train-mode forward (momentum 0.1, unbiased variance)"""
    unb = var * M / (M - 1) if M > 1 else var
    return (1 - MOMENTUM) * np.asarray(rm, np.float64) + MOMENTUM * mean, (1 - MOMENTUM) * np.asarray(rv, np.float64) + MOMENTUM * unb


def sample(z_mu, z_lv, bn_mu, bn_lv, eps, n_img, T):
    """gdl_dul_sample: bn_* = [>= 2][512] (scale, shift, ...).  Returns dict(mu, sd, out [M][512], f [B][512], reg)."""
    z_mu, z_lv, eps = (np.asarray(a, np.float64) for a in (z_mu, z_lv, eps))
    bn_mu, bn_lv = np.asarray(bn_mu, np.float64), np.asarray(bn_lv, np.float64)
    M = z_mu.shape[0]
    B, TP = n_img // T, M // (n_img // T)
    mu = z_mu * bn_mu[0] + bn_mu[1]
    lv = z_lv * bn_lv[0] + bn_lv[1]
    with np.errstate(over="ignore", invalid="ignore"):
        sd = np.exp(0.5 * lv)
        out = eps * sd + mu
        s2 = sd * sd
        t = 0.5 * (s2 + mu * mu - np.log(s2 + KL_EPS) - 1.0)
    return dict(mu=mu, lv=lv, sd=sd, out=out, t=t, f=out.reshape(B, TP, C).mean(1), reg=t.sum() / n_img)


def sample_bounds(r, eps, n_img, T, dtype_bytes):
    """(e_mu, e_sd, e_out [M][512], e_f [B][512], e_reg) for sample()'s result r"""
    mu, lv, sd, out, t = r["mu"], r["lv"], r["sd"], r["out"], r["t"]
    eps = np.abs(np.asarray(eps, np.float64))
    M = mu.shape[0]
    B, TP = n_img // T, M // (n_img // T)
    e_mu = U * np.abs(mu)
    r_sd = LIBM + 0.5 * U * np.abs(lv)
    e_out = eps * sd * r_sd + e_mu + U * np.abs(out)
    D = -(-TP // 16) + 16
    e_f = (e_out.reshape(B, TP, C).sum(1) + D * U * np.abs(out).reshape(B, TP, C).sum(1)) / TP + U * np.abs(r["f"])
    s2 = sd * sd
    la = np.abs(np.log(s2 + KL_EPS))
    e_t = 0.5 * ((2 * r_sd + U) * s2 + 3 * U * mu * mu + (2 * r_sd + 2 * U) + LIBM * la + 3 * U * (s2 + mu * mu + la + 1.0))
    blocks = B * (C // (16 // dtype_bytes) // 16)
    D = 8 * -(-TP // 16) + 8 + -(-blocks // 256) + 8
    e_reg = (e_t.sum() + D * U * np.abs(t).sum()) / n_img + U * abs(r["reg"])
    return SAFETY * e_mu, SAFETY * sd * r_sd, SAFETY * e_out, SAFETY * e_f, SAFETY * e_reg


# ---------------------------------------------------------------------------------------------------------------- backward
def grads(r, df, eps, beta, n_img, T):
    """(d_mu, d_lv) [M][512] from sample()'s result and the head's df [B][512]"""
    mu, sd = r["mu"], r["sd"]
    M = mu.shape[0]
    TP = M // (n_img // T)
    g = np.repeat(np.asarray(df, np.float64) / TP, TP, axis=0)
    k = beta / n_img
    with np.errstate(over="ignore", invalid="ignore"):
        d_mu = g + k * mu
        d_sd = g * np.asarray(eps, np.float64) + k * (sd - sd / (sd * sd + KL_EPS))
        return d_mu, d_sd * 0.5 * sd


def grad_bounds(r, df, eps, beta, n_img, T):
    """(e_dmu, e_dlv) for grads()"""
    mu, lv, sd = r["mu"], r["lv"], r["sd"]
    M = mu.shape[0]
    TP = M // (n_img // T)
    eps = np.abs(np.asarray(eps, np.float64))
    g = np.abs(np.repeat(np.asarray(df, np.float64) / TP, TP, axis=0))
    k = abs(beta / n_img)
    r_sd = LIBM + 0.5 * U * np.abs(lv)
    e_dmu = U * g + k * (U * np.abs(mu) + 2 * U * np.abs(mu)) + U * np.abs(g + k * np.abs(mu))
    q = sd / (sd * sd + KL_EPS)
    w = sd - q
    e_w = sd * r_sd + q * (3 * r_sd + 2 * U + LIBM) + U * np.abs(w)
    d_sd_mag = g * eps + k * np.abs(w)
    e_dsd = eps * U * g + k * (e_w + 3 * U * np.abs(w)) + U * d_sd_mag
    e_dlv = 0.5 * sd * e_dsd + 0.5 * sd * d_sd_mag * (r_sd + 2 * U)
    return e_dmu, e_dlv


def bn_backward(d, z, bn, gamma):
    """One stack's BatchNorm backward in the two-pass form: bn = [4][512] (scale, shift, mean, rstd).
    Returns dict(xhat, S1 (= dbeta), S2 (= dgamma), coef [2][512], dz)."""
    d, z, bn = np.asarray(d, np.float64), np.asarray(z, np.float64), np.asarray(bn, np.float64)
    M = z.shape[0]
    xhat = (z - bn[2]) * bn[3]
    S1, S2 = d.sum(0), (d * xhat).sum(0)
    coef = np.stack([S1 / M, S2 / M])
    dz = np.asarray(gamma, np.float64) * bn[3] * (d - coef[0] - xhat * coef[1])
    return dict(xhat=xhat, S1=S1, S2=S2, coef=coef, dz=dz)


def bn_backward_bounds(b, d, e_d, bn, gamma, rows_per_thread, dtype_bytes):
    """(e_S1, e_S2 [512], e_dz [M][512]) for bn_backward()'s result b; rows_per_thread: the most rows one thread of the
    reduce pass adds in sequence, ceil(vectors / (blocks 256))."""
    d, bn = np.abs(np.asarray(d, np.float64)), np.asarray(bn, np.float64)
    xh = np.abs(b["xhat"])
    M = xh.shape[0]
    e_xh = 2 * U * xh
    D = rows_per_thread + 4 + 1
    e_S1 = e_d.sum(0) + D * U * d.sum(0) + U * np.abs(b["S1"])
    e_S2 = (e_d * xh + d * (e_xh + U * xh)).sum(0) + D * U * (d * xh).sum(0) + U * np.abs(b["S2"])
    c0, c1 = np.abs(b["coef"][0]), np.abs(b["coef"][1])
    e_c0, e_c1 = e_S1 / M + U * c0, e_S2 / M + U * c1
    gr = np.abs(np.asarray(gamma, np.float64) * bn[3])
    e_dz = SAFETY * (gr * (e_d + e_c0 + xh * e_c1 + c1 * e_xh + 3 * U * (d + c0 + xh * c1)) + 2 * U * np.abs(b["dz"]))
    if dtype_bytes == 2:  # the store rounds the float32 value, which lies within e_dz of dz, to the nearest bfloat16
        e_dz = e_dz + 2 * U_BF16 * (np.abs(b["dz"]) + e_dz)
    return SAFETY * e_S1, SAFETY * e_S2, e_dz


def conv_backward(dz, x, W):
    """(dx [M][512] = dz W, dW [512][512] = dz^T x) of z = x W^T + b; db_conv is 0 (the named departure)"""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    return dz @ np.asarray(W, np.float64).reshape(C, C), dz.T @ x


# ---------------------------------------------------------------------------------------------------------------- eval
def eval_form(f, W, b, scale, shift):
    """gdl_dul_eval: out[b][k] = (W[k] . f[b] + bias[k]) scale[k] + shift[k]"""
    f, W = np.asarray(f, np.float64), np.asarray(W, np.float64).reshape(C, C)
    return (f @ W.T + np.asarray(b, np.float64)) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)


def eval_bound(f, W, b, scale, shift):
    f, W = np.asarray(f, np.float64), np.asarray(W, np.float64).reshape(C, C)
    dot_b = f @ W.T + np.asarray(b, np.float64)
    o = dot_b * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    D = 8 + 6
    return SAFETY * (np.abs(scale) * (D * U * (np.abs(f) @ np.abs(W).T) + U * np.abs(dot_b)) + U * np.abs(o))


def eval_scale_shift(gamma, beta, rm, rv):
    """gdl_bn_finalize_eval in float64"""
    sc = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(rv, np.float64) + BN_EPS)
    return sc, np.asarray(beta, np.float64) - np.asarray(rm, np.float64) * sc


# ---------------------------------------------------------------------------------------------------------------- whole stage
def stage(x, P, eps, df_fn, beta, n_img, T):
    """The whole branch of one encoder in float64.  P: the 8 tensors in registration order (mu conv weight, bias, mu BatchNorm
    weight, bias, then the logvar stack's four); df_fn(f) -> df [B][512], the head's feature gradient.  Returns a dict with the
    forward values, the 8 parameter gradients `dP` (the two convolution biases' exactly 0), dx and the batch statistics."""
    Wm, bm, gm, btm, Wl, bl, gl, btl = P
    M = np.asarray(x).shape[0]
    zm, scm, shm, mm, rm_, vm = conv_bn_train(x, Wm, bm, gm, btm)
    zl, scl, shl, ml, rl_, vl = conv_bn_train(x, Wl, bl, gl, btl)
    bn_mu, bn_lv = np.stack([scm, shm, mm, rm_]), np.stack([scl, shl, ml, rl_])
    r = sample(zm, zl, bn_mu, bn_lv, eps, n_img, T)
    df = df_fn(r["f"])
    d_mu, d_lv = grads(r, df, eps, beta, n_img, T)
    bm_, bl_ = bn_backward(d_mu, zm, bn_mu, gm), bn_backward(d_lv, zl, bn_lv, gl)
    dxm, dWm = conv_backward(bm_["dz"], x, Wm)
    dxl, dWl = conv_backward(bl_["dz"], x, Wl)
    r.update(z_mu=zm, z_lv=zl, bn_mu=bn_mu, bn_lv=bn_lv, var_mu=vm, var_lv=vl, df=df, dx=dxm + dxl, dz_mu=bm_["dz"], dz_lv=bl_["dz"],
             dP=[dWm.reshape(C, C, 1, 1), np.zeros(C), bm_["S2"], bm_["S1"], dWl.reshape(C, C, 1, 1), np.zeros(C), bl_["S2"], bl_["S1"]])
    return r


# ---------------------------------------------------------------------------------------------------------------- fixtures
DUL_NAMES = ("mu_dul_backbone.0.weight", "mu_dul_backbone.0.bias", "mu_dul_backbone.1.weight", "mu_dul_backbone.1.bias",
             "logvar_dul_backbone.0.weight", "logvar_dul_backbone.0.bias", "logvar_dul_backbone.1.weight", "logvar_dul_backbone.1.bias")


def dul_state(prefix):
    """Deterministic float32 state of one encoder's two stacks, ({name: parameter}, {name: buffer}) in state_dict order: Kaiming
    convolution weights, small biases, BatchNorm gamma around 1 and beta around 0 (the logvar stack's around -1: sd around 0.6)."""
    import zlib

    ps, bs = {}, {}
    for stack in ("mu_dul_backbone", "logvar_dul_backbone"):
        r = np.random.default_rng([zlib.crc32((prefix + stack).encode()), 7])
        ps[f"{prefix}{stack}.0.weight"] = (np.sqrt(2.0 / C) * r.standard_normal((C, C, 1, 1))).astype(np.float32)
        ps[f"{prefix}{stack}.0.bias"] = (0.01 * r.standard_normal(C)).astype(np.float32)
        ps[f"{prefix}{stack}.1.weight"] = (1.0 + 0.1 * r.standard_normal(C)).astype(np.float32)
        ps[f"{prefix}{stack}.1.bias"] = (0.1 * r.standard_normal(C) - (1.0 if stack[0] == "l" else 0.0)).astype(np.float32)
        bs[f"{prefix}{stack}.1.running_mean"] = (0.05 * r.standard_normal(C)).astype(np.float32)
        bs[f"{prefix}{stack}.1.running_var"] = (1.0 + 0.1 * np.abs(r.standard_normal(C))).astype(np.float32)
        bs[f"{prefix}{stack}.1.num_batches_tracked"] = np.zeros((), dtype=np.int64)
    return ps, bs


def golden_eps(n_img, P, seed, step, modality):
    """The noise the step goldens inject: the generator's normals as the float32 [n_img P][512] map `step(..., pe_eps=)` takes"""
    return normals(n_img * P * C, seed, step, modality).reshape(n_img * P, C).astype(np.float32)
