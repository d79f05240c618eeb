"""CPU-only checks of the BatchNorm accumulator arithmetic (csrc/bnacc.h): the host query gdl_bn_acc_scales against its
restatement, the restated chain partial rows -> accumulators -> constants (tests/bnacc_ref.py, what tests/test_bnacc_gpu.py
holds the kernels to) against the oracle's BatchNorm, and the headroom statement of bnacc.h."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bnacc_ref as ref  # noqa: E402
from gdl import _lib as L  # noqa: E402

from oracle import oracle as orc  # noqa: E402

# 1, 2, 3, 2^k and 2^k + 1 (L steps right after a power of two), the stem output of the B = 64 visual batch (602 112 rows),
# and counts beyond 2^36: there 62 - 26 - L < 0 and s2 is a reciprocal
ROWS = [1, 2, 3] + [v for k in (2, 5, 10, 16, 19, 20, 31, 32, 35, 36) for v in (1 << k, (1 << k) + 1)] + [602112, (1 << 37) + 5, 1 << 40]


def test_scales_match_the_library():
    lib = L.load()
    for rows in ROWS:
        s1, s2 = ctypes.c_double(), ctypes.c_double()
        assert lib.gdl_bn_acc_scales(rows, ctypes.byref(s1), ctypes.byref(s2)) == 0
        assert (s1.value, s2.value) == ref.scales(rows), rows
    # the values themselves, where the exponent steps: L = ceil(log2(rows))
    assert ref.scales(1) == (2.0 ** 49, 2.0 ** 36) and ref.scales(2) == (2.0 ** 48, 2.0 ** 35)
    assert ref.scales(3) == ref.scales(4) == (2.0 ** 47, 2.0 ** 34) and ref.scales(5) == (2.0 ** 46, 2.0 ** 33)
    assert ref.scales(602112) == (2.0 ** 29, 2.0 ** 16)
    assert ref.scales((1 << 36) + 1) == (2.0 ** 12, 0.5) and ref.scales(1 << 40) == (2.0 ** 9, 2.0 ** -4)
    assert lib.gdl_bn_acc_scales(0, None, None) != 0 and lib.gdl_last_error()


def test_headroom_statement():
    """bnacc.h: "exact headroom for |y| < 8192".  rows values of magnitude below 2^13 sum to less than rows 2^13 and their squares
    to less than rows 2^26; times the scale that must stay below 2^62 -- in exact rational arithmetic, at every row count of the
    sweep: rows 2^13 s1 <= 2^62 and rows 2^26 s2 <= 2^62 (strictness comes from |y| < 8192 being strict)."""
    for rows in ROWS:
        s1, s2 = (Fraction(v) for v in ref.scales(rows))
        assert rows * 2 ** 13 * s1 <= 2 ** 62 and rows * 2 ** 26 * s2 <= 2 ** 62, rows
        # and no bit is given away: half the scale's headroom would not hold twice the rows
        assert 2 * rows * 2 ** 13 * s1 > 2 ** 62 or rows == 1


@pytest.mark.parametrize("shape,tile", [((3, 8, 7, 5), 16), ((2, 4, 33, 31), 128), ((1, 6, 1, 1), 1), ((5, 3, 2, 3), 7)])
def test_reference_chain_against_the_oracle(shape, tile):
    """partial rows -> acc_from_partials -> channel_constants against oracle.bn_fwd_train on the same data.
    The data are multiples of 1/8 in [-8, 8): every tile sum and every sum of squares is exact in float64, so the ONLY error of the
    chain is the fixed-point rounding, at most half a unit per tile and word:
        |mean error| <= tiles 0.5 / (s1 count) =: dm,     |second-moment error| <= tiles 0.5 / (s2 count) =: dq
    The oracle returns float32 (one rounding of a double result: 2^-24 relative, its own error), and it returns rstd, not the
    second moment: var = q - mean^2 moves by at most dv = dq + 2 |mean| dm + dm^2, rstd = (var + eps)^-1/2 by at most
    rstd^3 dv / 2 to first order (the factor 1.01 covers the second order: dv / (var + eps) is below 1e-3 here)."""
    N, C, H, W = shape
    rng = np.random.default_rng(7)
    x = (rng.integers(-64, 64, size=shape) / 8.0).astype(np.float32)
    x[:, 0] = 0.375  # a constant channel: variance exactly 0
    if C > 2:
        x[:, 2] -= 5.0  # a negative mean of several standard deviations
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    gamma[-1] *= -1
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    rm0, rv0 = (0.05 * rng.standard_normal(C)).astype(np.float32), (1 + 0.1 * rng.random(C)).astype(np.float32)
    rows = N * H * W
    xr = np.transpose(x, (0, 2, 3, 1)).reshape(rows, C).astype(np.float64)
    tiles = -(-rows // tile)
    part = np.zeros((tiles, C, 2))
    for t in range(tiles):
        blk = xr[t * tile:(t + 1) * tile]
        part[t, :, 0], part[t, :, 1] = blk.sum(0), (blk * blk).sum(0)
    s1, s2 = ref.scales(rows)
    acc = ref.acc_from_partials(part, s1, s2)
    assert acc.dtype == np.int64 and acc.shape == (C, 2)
    k = ref.channel_constants(acc, 1.0 / s1, 1.0 / s2, rows, gamma, beta, 1e-5, 0.1, rm0, rv0)
    rm, rv = rm0.copy(), rv0.copy()
    _, mean, invstd = orc.bn_fwd_train(x, gamma, beta, rm, rv)
    u = 2.0 ** -24
    dm, dq = tiles * 0.5 / (s1 * rows), tiles * 0.5 / (s2 * rows)
    # the second moment against plain float64 (exact on these data), then the oracle's outputs
    assert np.all(np.abs(acc[:, 1] / s2 / rows - (xr * xr).sum(0) / rows) <= dq)
    assert np.all(np.abs(acc[:, 0] / s1 / rows - xr.sum(0) / rows) <= dm)
    assert np.all(np.abs(k["mean"] - mean) <= dm + u * np.abs(mean))
    dv = dq + 2 * np.abs(k["mean"]) * dm + dm * dm
    drstd = 1.01 * 0.5 * k["rstd"] ** 3 * dv
    assert np.all(np.abs(k["rstd"] - invstd) <= drstd + u * np.abs(invstd)), (np.abs(k["rstd"] - invstd).max(), drstd.max())
    assert np.all(np.abs(k["running_mean"] - rm) <= 0.1 * dm + u * np.abs(rm))
    unb = rows / (rows - 1.0) if rows > 1 else 1.0
    assert np.all(np.abs(k["running_var"] - rv) <= 0.1 * unb * dv + u * np.abs(rv))
    # scale / shift follow from mean and rstd: exact restatement
    np.testing.assert_array_equal(k["scale"], gamma.astype(np.float64) * k["rstd"])
    np.testing.assert_array_equal(k["shift"], beta.astype(np.float64) - k["mean"] * gamma.astype(np.float64) * k["rstd"])
    assert k["rstd"][0] == 1.0 / np.sqrt(float(np.float32(1e-5)))  # the constant channel: variance exactly 0


def test_clamp_flag_and_guard_of_the_reference():
    s1, s2 = ref.scales(100)
    # a second moment below mean^2 (tile roundings can leave it there): the variance is clamped at 0, not negative
    acc = np.array([[int(100 * 3.0 * s1), int(100 * 9.0 * s2) - int(1e-6 * 100 * s2)]], dtype=np.int64)
    k = ref.channel_constants(acc, 1 / s1, 1 / s2, 100, [1.0], [0.0], 1e-5, 0.1, [0.0], [1.0])
    assert k["rstd"][0] == 1.0 / np.sqrt(float(np.float32(1e-5))) and k["running_var"][0] == 1.0 - float(np.float32(0.1))
    k = ref.channel_constants(acc, 1 / s1, 1 / s2, 100, [1.0], [0.0], 1e-5, 0.1, [0.0], [1.0], flag=1)
    assert all(np.isnan(k[n][0]) for n in ("mean", "rstd", "scale", "shift", "running_mean", "running_var"))
    # the guard: rows at or beyond the block's share are left out and reported; half-way cases round to even
    part = np.array([[[1.0, 2.0]], [[np.inf, 3.0]], [[np.nan, 4.0e30]], [[2.5, 0.5]]])
    a, flag = ref.acc_from_partials(part, 1.0, 1.0, grid=4)
    assert flag == 1 and a.tolist() == [[3, 5]]  # 1 + rint(2.5) = 3;  2 + 3 + rint(0.5) = 5
    a, flag = ref.acc_from_partials(part[[0, 3]], 1.0, 1.0, grid=4)
    assert flag == 0 and a.tolist() == [[3, 2]]
    assert ref.acc_from_partials(part[[0, 3]], 2.0, 4.0).tolist() == [[7, 10]]
