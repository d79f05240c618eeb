"""float64 NumPy restatement of the MMPareto gradient integration (csrc/pareto.hip): one encoder's gradient
of the fused loss, g_m, and of its own weighted unimodal loss, g_u, as one vector each.

    S_mm = sum g_m^2,  S_uu = sum g_u^2,  S_mu = sum g_m g_u                                  (float32 data, double sums)
    S_mu > 0 and all three finite (agreement, branch 1):
        D = S_mm - 2 S_mu + S_uu;  gamma = D > 0 ? clamp((S_uu - S_mu) / D, 0, 1) : 0.5       (the min-norm point of [g_u, g_m];
        w_m = 2 gamma,  w_u = 2 (1 - gamma)                                                    gamma weighs g_m)
        N_h^2 = w_m^2 S_mm + 2 w_m w_u S_mu + w_u^2 S_uu;   N_s^2 = S_mm + 2 S_mu + S_uu
        s = N_h^2 > 0 and finite ? sqrt(N_s^2 / N_h^2) : 1
    otherwise (sum, branch 0):  gamma = 0.5,  w_m = w_u = 1,  s = 1
    c_m = float32(scale s w_m),  c_u = float32(scale s w_u);   g = c_u g_u + c_m g_m
"""
import numpy as np

INFO_KEYS = ("S_mm", "S_uu", "S_mu", "gamma", "w_m", "w_u", "s", "branch")
U = 2.0 ** -24


def sums(g_m, g_u):
    """(S_mm, S_uu, S_mu) in float64: the products of float32 values are exact in float64, numpy's pairwise sum of them is within
    n 2^-53 (relative to the sum of the terms' magnitudes) of the exact sum -- and, a function of the terms alone, it gives equal
    vectors three equal sums (D = 0 exactly, as on the device)"""
    a, b = np.asarray(g_m, dtype=np.float64).ravel(), np.asarray(g_u, dtype=np.float64).ravel()
    return float(np.sum(a * a)), float(np.sum(b * b)), float(np.sum(a * b))


def coefficients(S_mm, S_uu, S_mu, scale=1.0):
    """dict of INFO_KEYS (float64; branch int) plus gamma_raw (the unclamped quotient, None outside the agreement branch or at
    D <= 0), c_m and c_u (rounded to float32, returned as float64)"""
    S_mm, S_uu, S_mu = float(S_mm), float(S_uu), float(S_mu)
    fin = np.isfinite(S_mm) and np.isfinite(S_uu) and np.isfinite(S_mu)
    gamma, w_m, w_u, s, branch, raw = 0.5, 1.0, 1.0, 1.0, 0, None
    if fin and S_mu > 0.0:
        branch = 1
        D = S_mm - 2.0 * S_mu + S_uu
        if D > 0.0:
            raw = (S_uu - S_mu) / D
            gamma = min(max(raw, 0.0), 1.0)
        w_m, w_u = 2.0 * gamma, 2.0 * (1.0 - gamma)
        Nh2 = w_m * w_m * S_mm + 2.0 * w_m * w_u * S_mu + w_u * w_u * S_uu
        Ns2 = S_mm + 2.0 * S_mu + S_uu
        if Nh2 > 0.0 and np.isfinite(Nh2):
            s = float(np.sqrt(Ns2 / Nh2))
    scale = float(np.float32(scale))
    return dict(S_mm=S_mm, S_uu=S_uu, S_mu=S_mu, gamma=gamma, w_m=w_m, w_u=w_u, s=s, branch=branch, gamma_raw=raw,
                c_m=float(np.float32(scale * s * w_m)), c_u=float(np.float32(scale * s * w_u)))


def integrate(g_m, g_u, scale=1.0):
    """(g float64, coefficients dict): the integrated gradient with the float32-rounded coefficients, evaluated in float64"""
    c = coefficients(*sums(g_m, g_u), scale=scale)
    with np.errstate(invalid="ignore"):
        g = c["c_u"] * np.asarray(g_u, dtype=np.float64) + c["c_m"] * np.asarray(g_m, dtype=np.float64)
    return g, c


def combine(g_m, g_u, c_m, c_u):
    """c_u g_u + c_m g_m in float64 for given (e.g. the device's own) coefficients"""
    with np.errstate(invalid="ignore"):
        return float(c_u) * np.asarray(g_u, dtype=np.float64) + float(c_m) * np.asarray(g_m, dtype=np.float64)
