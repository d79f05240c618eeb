"""Float64 NumPy statement of the feature-diversity monitor (csrc/diversity.hip, gdl.feature_diversity), the project's own
reading of main.py:77-89, and the seeded maps its tests run on.  Per image, x_p = the C channels at position p (P = h w):

    c_p = x_p - mean_C(x_p);  s_p = sqrt(sum_C c_p^2 / (C - 1));  R_pq = (c_p . c_q) / (s_p s_q);  d = ||R||_F / P^2

A position whose channels are all equal has s_p = 0: 0 / 0 = NaN for that image (and for the mean over the images).
"""
import numpy as np

C = 512
KINDS = ("relu", "shift32", "same", "zero_row")
# the op shapes of the tests and of the golden file: (n_img, h, w)
SHAPES = ((1, 1, 1), (3, 2, 2), (2, 3, 2), (5, 4, 4), (2, 17, 1), (3, 7, 7), (2, 9, 6), (2, 5, 20), (1, 16, 16), (300, 2, 2))
SAME_SHAPE = (2, 7, 7)
ZERO_ROW = (1, 11)  # zero_row: this (image, position) is zeroed (clipped to the map's size)


def diversity_ref(fmap):
    """fmap [N, C, h, w] (any float dtype) -> (per-image d [N] float64, their mean); float64 throughout"""
    x = np.asarray(fmap, dtype=np.float64)
    n, c = x.shape[:2]
    x = x.reshape(n, c, -1).transpose(0, 2, 1)  # [N, P, C]
    p = x.shape[1]
    cen = x - x.mean(axis=2, keepdims=True)
    std = np.sqrt((cen ** 2).sum(axis=2) / (c - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.einsum("npc,nqc->npq", cen, cen) / (std[:, :, None] * std[:, None, :])
    d = np.sqrt((r ** 2).sum(axis=(1, 2))) / p ** 2
    return d, d.mean()


def zero_row_index(n_img, h, w):
    return min(ZERO_ROW[0], n_img - 1), min(ZERO_ROW[1], h * w - 1)


def make_map(seed, n_img, h, w, kind):
    """[n_img, 512, h, w] float32, regenerated from (seed, shape, kind) -- nothing is stored.
    relu: max(N(0,1) + 0.3 (per-channel offset), 0), a post-ReLU map;  shift32: N(0,1) + 32 (a mean 32 standard deviations
    off zero: what a raw-moment form must survive);  same: every position of an image equal;  zero_row: relu with all 512
    channels of one position of one image zero."""
    assert kind in KINDS
    r = np.random.default_rng([seed, n_img, h, w, KINDS.index(kind)])
    if kind == "shift32":
        return (r.standard_normal((n_img, C, h, w)) + 32.0).astype(np.float32)
    if kind == "same":
        return np.broadcast_to(r.standard_normal((n_img, C, 1, 1)), (n_img, C, h, w)).astype(np.float32)
    off = r.standard_normal((1, C, 1, 1))
    x = np.maximum(r.standard_normal((n_img, C, h, w)) + 0.3 * off, 0.0).astype(np.float32)
    if kind == "zero_row":
        i, p = zero_row_index(n_img, h, w)
        x.reshape(n_img, C, h * w)[i, :, p] = 0.0
    return x


def fold_mean(vals):
    """The kernel's mean of n float32 terms, in ITS order: 256 partial sums taking i, i + 256, ... in turn, folded as the tree
    p[i] += p[i + o], o = 128 .. 1; then one division by n -- float32 throughout."""
    v = np.asarray(vals, dtype=np.float32)
    p = np.zeros(256, dtype=np.float32)
    for i0 in range(0, len(v), 256):
        blk = v[i0:i0 + 256]
        p[:len(blk)] += blk
    o = 128
    while o:
        p[:o] = p[:o] + p[o:2 * o]
        o >>= 1
    return np.float32(p[0] / np.float32(len(v)))
