"""float64 NumPy restatement of OGM / OGM-GE gradient modulation (main.py:286-330 and the published OGM-GE code) as
csrc/optim.hip and csrc/head.hip compute it: the Philox4x32-10 generator, its uniforms, Box-Muller, the unimodal scores, the two
coefficients and the modulation of a flat arena.  The yardstick of tests/test_modulation_gpu.py, itself pinned by
tests/test_modulation_cpu.py (known-answer vectors, moments, a torch restatement).  No GPU, no reference import."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays.
    Round: c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key grows by (W0, W1) per round."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in np.broadcast_arrays(*ctr))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)), p1 & np.uint64(MASK),
                          ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)), p0 & np.uint64(MASK))
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform(w):
    """u(w) = ((w >> 8) + 0.5) 2^-24, in (0, 1)"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def box_muller(wa, wb):
    r = np.sqrt(-2.0 * np.log(uniform(wa)))
    th = 2.0 * np.pi * uniform(wb)
    return r * np.cos(th), r * np.sin(th)


def normals(index, seed, step):
    """The standard normal of arena element `index` (an int64 array) at `step` under `seed`: counter (i >> 2, 0, step, 0), key
    (seed low, seed high); words (0, 1) give z0, z1, words (2, 3) give z2, z3; element i takes z[i & 3]."""
    index = np.asarray(index, dtype=np.int64)
    q = index >> 2
    w = philox4x32_10((q & MASK, q >> 32, np.full_like(q, step & MASK), np.full_like(q, (step >> 32) & MASK)),
                      (seed & MASK, (seed >> 32) & MASK))
    z = np.stack(box_muller(w[0], w[1]) + box_muller(w[2], w[3]))
    return np.take_along_axis(z, (index & 3)[None], axis=0)[0]


def label_probs(logits, label):
    """softmax(logits)[i, label_i], float64"""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e[np.arange(len(label)), label] / e.sum(axis=1)


def uni_logits(head, fa, fv, P):
    """The published unimodal logits from the pooled features: concat (P = fc_out weight [n, 1024], bias) -- a W[:, :512]^T + b/2,
    v W[:, 512:]^T + b/2; sum (P = fc_x weight, bias, fc_y weight, bias) -- fc_x(a), fc_y(v)."""
    fa, fv = np.asarray(fa, np.float64), np.asarray(fv, np.float64)
    P = [np.asarray(p, np.float64) for p in P]
    if head == "concat":
        return fa @ P[0][:, :512].T + P[1] / 2, fv @ P[0][:, 512:].T + P[1] / 2
    return fa @ P[0].T + P[1], fv @ P[2].T + P[3]


def coefficients(score_a, score_v, alpha):
    """(ratio_v, coeff_a, coeff_v): the side that leads is slowed by 1 - tanh(alpha * its ratio); ratio_v == 1 takes the audio
    branch (main.py:296-301)."""
    ratio_v = score_v / score_a
    if ratio_v > 1:
        return ratio_v, 1.0, 1.0 - np.tanh(alpha * ratio_v)
    return ratio_v, 1.0 - np.tanh(alpha * (1.0 / ratio_v)), 1.0


def sigma(gk):
    """std(g) + 1e-8 of a clipped tensor: torch's unbiased standard deviation"""
    return float(np.std(np.asarray(gk, np.float64), ddof=1)) + 1e-8


def modulate(g, offsets, marks, k, coeff_a, coeff_v, noise, seed=0, step=0):
    """g: the float32 arena before the clip; k: the float32 factor clip_coef * grad_scale.  Returns (the modulated arena in
    float64 built from float32(g k), per-segment sigma): marked segments (g k) c [+ sigma z], unmarked ones g k."""
    gk = (np.asarray(g, np.float32) * np.float32(k)).astype(np.float64)
    out, sig = gk.copy(), np.zeros(len(marks))
    for s, m in enumerate(marks):
        if not m:
            continue
        b, e = int(offsets[s]), int(offsets[s + 1])
        out[b:e] = gk[b:e] * (coeff_a if m == 1 else coeff_v)
        if noise:
            sig[s] = sigma(gk[b:e])
            out[b:e] += sig[s] * normals(np.arange(b, e, dtype=np.int64), seed, step)
    return out, sig
