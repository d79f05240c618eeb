"""float64 NumPy / Python-int restatement of the BatchNorm accumulator path (csrc/bnacc.h) and of the fused block backward
(csrc/bn.hip block_bwd_reduce_kernel, bn_bwd_apply2_kernel).

Forward statistics: a convolution epilogue turns each tile's two per-channel float32 sums into fixed point and adds them to
int64 acc[C][2] (+ one flag word),

    acc[c][w] += rint(sum_w * s_w),   s_1 = 2^(49 - L), s_2 = 2^(36 - L), L = ceil(log2(rows))          (scales)

unless |sum_w * s_w| >= 4.6e18 / grid (or is NaN / inf): that block adds nothing and sets the flag.  The consumer derives, in
double, per channel

    mean = acc[c][0] / s_1 / count,  var = max(acc[c][1] / s_2 / count - mean^2, 0),  rstd = 1 / sqrt(var + eps)
    scale = gamma rstd,  shift = beta - mean gamma rstd,  running <- (1 - m) running + m {mean, var count / (count - 1)}

and publishes them rounded to float32 (NaN when the flag is set).
"""
import numpy as np

GUARD = 4.6e18  # bn_acc_add: a block's share of the range is GUARD / grid


def scales(rows):
    """(s1, s2) of bn_acc_scales: L = the smallest integer with 2^L >= rows"""
    rows = int(rows)
    L = max(rows - 1, 0).bit_length()
    return 2.0 ** (62 - 13 - L), 2.0 ** (62 - 26 - L)  # (a negative exponent: the reciprocal branch, exact as well)


def acc_from_partials(part, s1, s2, grid=None):
    """part [rows][C][2] (float32 partial rows, or float64) -> int64 [C][2] = sum_rows rint(part[row][c][w] * s_w).
    np.rint rounds half to even like __double2ll_rn; a float32 times a power of two is exact in float64.
    grid (optional): apply the guard of bn_acc_add with that block count -- rows whose |value| is not below GUARD / grid (NaN
    and inf included) are left out; then returns (acc, flag) with flag = 1 when any row was."""
    v = np.asarray(part, dtype=np.float64) * np.array([s1, s2], dtype=np.float64)
    if grid is None:
        return np.rint(v).astype(np.int64).sum(axis=0)
    with np.errstate(invalid="ignore"):
        ok = np.abs(v) < GUARD / float(grid)  # (False for NaN)
    q = np.where(ok, np.rint(np.where(ok, v, 0.0)), 0.0).astype(np.int64)
    return q.sum(axis=0), int(not ok.all())


def channel_constants(acc, inv_s1, inv_s2, count, gamma, beta, eps, momentum, rm=None, rv=None, flag=0):
    """bn_acc_channel in its own order.  acc int64 [C][2]; gamma / beta / rm / rv float32 [C]; eps / momentum are float32 on
    the device.  Returns a dict of float64 [C] arrays BEFORE the rounding to float32: mean, rstd, scale, shift and, with
    rm / rv, running_mean, running_var."""
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, 2)
    count = float(count)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    s = acc[:, 0].astype(np.float64) * inv_s1
    q = acc[:, 1].astype(np.float64) * inv_s2
    if flag:
        s = np.full_like(s, np.nan)
    with np.errstate(invalid="ignore"):
        mean = s / count
        var = q / count - mean * mean  # biased
        var = np.where(var < 0.0, 0.0, var)  # (NaN stays NaN: the comparison is false)
        rstd = 1.0 / np.sqrt(var + eps)
        g = np.asarray(gamma, dtype=np.float64)
        out = {"mean": mean, "rstd": rstd, "scale": g * rstd, "shift": np.asarray(beta, dtype=np.float64) - mean * g * rstd}
        if rm is not None:
            unb = var * count / (count - 1.0) if count > 1.0 else var
            out["running_mean"] = (1.0 - momentum) * np.asarray(rm, dtype=np.float64) + momentum * mean
            out["running_var"] = (1.0 - momentum) * np.asarray(rv, dtype=np.float64) + momentum * unb
    return out


def block_bwd_reduce(dz, z, y2, yd, mean2, rstd2, meand, rstdd, premasked):
    """[M][C] tensors, float64 arithmetic.  Returns (do2, sums2 [C][2], sumsd [C][2] or None, abs2 [C][2], absd [C][2] or None):
    do2 = premasked ? dz : where(z > 0, dz, 0); sums = { sum do2, sum do2 (y - mean) rstd } over the rows; abs* = the same sums
    over the terms' magnitudes (what an error bound of the float32 accumulation scales with)."""
    g = np.asarray(dz, dtype=np.float64)
    if not premasked:
        g = np.where(np.asarray(z) > 0, g, 0.0)

    def side(y, mean, rstd):
        t = g * ((np.asarray(y, dtype=np.float64) - np.asarray(mean, dtype=np.float64)[None, :]) * np.asarray(rstd, dtype=np.float64)[None, :])
        return np.stack([g.sum(0), t.sum(0)], axis=1), np.stack([np.abs(g).sum(0), np.abs(t).sum(0)], axis=1)

    s2, a2 = side(y2, mean2, rstd2)
    sd, ad = side(yd, meand, rstdd) if yd is not None else (None, None)
    return g, s2, sd, a2, ad


def bn_bwd_apply(g, y, mean, rstd, gamma, coef):
    """dy = gamma rstd (g - coef[0] - (y - mean) rstd coef[1]) in float64, and the magnitude the float32 evaluation's error
    scales with: |gamma rstd| (|g| + |coef[0]| + |(y - mean) rstd coef[1]|).  coef [2][C]."""
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mean, rstd, gamma = (np.asarray(v, dtype=np.float64)[None, :] for v in (mean, rstd, gamma))
    k = np.asarray(coef, dtype=np.float64).reshape(2, -1)
    c = (y - mean) * rstd * k[1][None, :]
    return gamma * rstd * (g - k[0][None, :] - c), np.abs(gamma * rstd) * (np.abs(g) + np.abs(k[0])[None, :] + np.abs(c))


def bn_bwd_apply2(g, yA, meanA, rstdA, gammaA, coefA, yB, meanB, rstdB, gammaB, coefB):
    """the two BatchNorms fed by one gradient: ((dyA, magA), (dyB, magB))"""
    return bn_bwd_apply(g, yA, meanA, rstdA, gammaA, coefA), bn_bwd_apply(g, yB, meanB, rstdB, gammaB, coefB)
