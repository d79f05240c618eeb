"""The element-wise convolution checker tested by itself, without a GPU: conv_ref's references against the oracle, the bound against
an fp32-accumulated CPU result for every case the GPU file runs, seeded corruptions that must fail (two of which the old norm-wise
criterion lets through -- the gap the element-wise tests close), and the guard bands."""
import functools

import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_ref as cr
from oracle import oracle as orc

rng = np.random.default_rng(77)


# ---------------------------------------------------------------- the references against the oracle's float32 functions
@pytest.mark.parametrize("geo", [(2, 5, 9, 7, 6, 3, 1, 1), (2, 4, 11, 7, 6, 3, 2, 1), (3, 4, 9, 6, 5, 1, 2, 0), (1, 3, 8, 10, 4, 3, 2, 1)])
def test_references_agree_with_the_oracle(geo):
    N, C, H, W, K, R, stride, pad = geo
    x = rng.standard_normal((N, C, H, W), dtype=np.float32)
    w = rng.standard_normal((K, C, R, R), dtype=np.float32)
    ref, mag = cr.conv_fwd(x, w, stride, pad)
    assert cr.relerr(orc.conv2d_fwd(x, w, stride, pad), ref) < 1e-6
    assert cr.relerr(orc.conv2d_fwd(np.abs(x), np.abs(w), stride, pad), mag) < 1e-6 and np.all(mag >= np.abs(ref))
    dy = rng.standard_normal(ref.shape, dtype=np.float32)
    fn = cr.conv_dgrad_s1 if stride == 1 else cr.conv_dgrad_s2
    dref, dmag = fn(dy, w, (H, W), pad)
    assert dref.shape == (N, C, H, W)
    assert cr.relerr(orc.conv2d_bwd_data(dy, w, (N, C, H, W), stride, pad), dref) < 1e-6
    assert cr.relerr(orc.conv2d_bwd_data(np.abs(dy), np.abs(w), (N, C, H, W), stride, pad), dmag) < 1e-6


@pytest.mark.parametrize("geo", [(2, 4, 11, 7, 6), (2, 4, 8, 10, 5)])
def test_downsample_pair_agrees_with_the_oracle(geo):
    N, C, H, W, K = geo
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w, wds = rng.standard_normal((K, C, 3, 3), dtype=np.float32), rng.standard_normal((K, C, 1, 1), dtype=np.float32)
    dy, dyd = rng.standard_normal((N, K, P, Q), dtype=np.float32), rng.standard_normal((N, K, P, Q), dtype=np.float32)
    ref, mag = cr.conv_dgrad_ds(dy, w, dyd, wds, (H, W))
    want = orc.conv2d_bwd_data(dy, w, (N, C, H, W), 2, 1).astype(np.float64) + orc.conv2d_bwd_data(dyd, wds, (N, C, H, W), 2, 0)
    assert cr.relerr(want, ref) < 1e-6 and np.all(mag >= np.abs(ref))


@pytest.mark.parametrize("geo", [(2, 1, 1, 9, 14), (1, 3, 2, 11, 13)])
def test_stem_reference_agrees_with_the_oracle(geo):
    B, Cin, T, H, W = geo
    x = rng.standard_normal(geo, dtype=np.float32)
    w = rng.standard_normal((64, Cin, 7, 7), dtype=np.float32)
    ref, mag = cr.stem_fwd(x, w)
    x4 = np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4)).reshape(B * T, Cin, H, W)
    assert cr.relerr(orc.conv2d_fwd(x4, w, 2, 3), ref) < 1e-6 and np.all(mag >= np.abs(ref))


# ---------------------------------------------------------------- the bound against a correct result, for the whole shared case list
@functools.lru_cache(maxsize=2)
def _built(cid):
    case = cc.BY_ID[cid]
    inp = cc.make_inputs(case)
    ref64, bnd, zero = cc.reference(case, inp)
    fx = cc.fixture(case, inp)
    for a in (ref64, bnd, fx):
        a.setflags(write=False)
    return case, inp, ref64, bnd, zero, fx


@pytest.mark.parametrize("cid", [c.id for c in cc.CASES])
def test_fp32_accumulated_result_is_inside_the_bound(cid):
    """torch's float32 convolution of the quantised inputs + extras, rounded once: what a correct kernel computes."""
    case, inp, ref64, bnd, zero, fx = _built(cid)
    assert cr.check(fx, ref64, bnd, zero_where=zero) <= 1.0
    if case.dt == "bf16":  # and the bound is not slack: one bf16 rounding nearly exhausts it somewhere
        assert cr.check(fx, ref64, bnd, zero_where=zero) > 0.3


# ---------------------------------------------------------------- seeded corruptions
TAP_CASES = ["c64_dgrad_ragged", "ps128_dgrad_odd", "c64_fwd_ragged", "flat_bf16_64_fwd_s2_odd"]


def _fails(got, ref64, bnd, zero=None):
    with pytest.raises(AssertionError) as e:
        cr.check(got, ref64, bnd, zero_where=zero)
    return str(e.value)


@pytest.mark.parametrize("cid", TAP_CASES)
def test_one_element_off_by_three_bounds_fails_but_passes_the_old_criterion(cid):
    case, inp, ref64, bnd, zero, fx = _built(cid)
    got = fx.astype(np.float64)
    n, c, h, w = (s // 2 for s in got.shape)
    got[n, c, h, w] = ref64[n, c, h, w] + 3.0 * bnd[n, c, h, w]
    msg = _fails(got, ref64, bnd)
    assert "1 of" in msg and f"(n={n}, c={c}, h={h}, w={w})" in msg
    assert cr.relerr(got, ref64) < cc.OLD_LIMIT[case.op]


@pytest.mark.parametrize("cid", TAP_CASES)
def test_missing_tap_in_a_corner_fails_but_passes_the_old_criterion(cid):
    """One tap of nine dropped in 16 channels of the corner pixel (0, 0) of image 0 -- a wrong tap mask, tile tail or slab shift.  The
    dropped tap is the one that reads the image's second row (the first is ten times as loud: even the norm would notice that)."""
    case, inp, ref64, bnd, zero, fx = _built(cid)
    w = inp["w"].astype(np.float64)
    if case.op == "fwd":   # y[0, k, 0, 0] += sum_c x[0, c, -pad + r, -pad + s] w[k, c, r, s]: r = 2, s = 1 reads x[.., 1, 0]
        tap = w[:16, :, 2, 1] @ inp["x"][0, :, 1, 0].astype(np.float64)
    else:                  # dx[0, c, 0, 0] += sum_k dy[0, k, pad - r, pad - s] w[k, c, r, s]: r = 0, s = 1 reads dy[.., 1, 0]
        assert case.shape[6] == 1
        tap = inp["dy"][0, :, 1, 0].astype(np.float64) @ w[:, :16, 0, 1]
    got = fx.copy()
    got[0, :16, 0, 0] = cc.quant((fx[0, :16, 0, 0] - tap).astype(np.float32), case.dt)
    msg = _fails(got, ref64, bnd)
    assert "border=yes" in msg and "row=0 " in msg
    with pytest.raises(AssertionError):
        cr.check(got[:, :16, :1, :1], ref64[:, :16, :1, :1], bnd[:, :16, :1, :1])
    worst = float((np.abs(got - ref64) / bnd)[0, :16, 0, 0].max())
    assert worst > 10.0, worst  # far outside, not marginally
    assert cr.relerr(got, ref64) < cc.OLD_LIMIT[case.op], cr.relerr(got, ref64)  # the old test would have passed


@pytest.mark.parametrize("cid", TAP_CASES)
def test_swapped_channels_fail(cid):
    case, inp, ref64, bnd, zero, fx = _built(cid)
    got = fx.copy()
    n, h, w = got.shape[0] - 1, got.shape[2] // 3, got.shape[3] // 2
    got[n, [4, 5], h, w] = got[n, [5, 4], h, w]
    assert "2 of" in _fails(got, ref64, bnd)


@pytest.mark.parametrize("cid", ["c64_dgrad_ragged", "ps128_fwd_odd", "c64_dgrad_addend", "ps128_dgrad_rich_addend"])
def test_vector_of_the_ragged_last_tile_left_at_its_fill_fails(cid):
    """The last 16-byte channel vector of the last GEMM row never stored: it keeps the output's NaN fill, or the addend of an
    in-place launch."""
    case, inp, ref64, bnd, zero, fx = _built(cid)
    got = fx.copy()
    got[-1, -8:, -1, -1] = inp["add"][-1, -8:, -1, -1] if "add" in inp else np.nan
    msg = _fails(got, ref64, bnd)
    N, C, H, W = got.shape
    assert f"row={N * H * W - 1} " in msg


def test_relu_zero_is_exact():
    case, inp, ref64, bnd, zero, fx = _built("slab_bf16_128x64_dgrad_relu")
    assert zero.any() and cr.check(fx, ref64, bnd, zero_where=zero) <= 1.0
    got = fx.copy()
    n, c, h, w = np.argwhere(zero)[7]
    got[n, c, h, w] = 1e-30  # inside any bound, but not the exact zero a cleared bit stores
    assert cr.check(got, ref64, bnd) <= 1.0
    assert f"(n={n}, c={c}, h={h}, w={w})" in _fails(got, ref64, bnd, zero)


def test_check_layout_nhwc():
    case, inp, ref64, bnd, zero, fx = _built("slab_bf16_128x64_fwd")
    t = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
    assert cr.check(t(fx), t(ref64), t(bnd), layout="nhwc") == cr.check(fx, ref64, bnd)


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
@pytest.mark.parametrize("poison", ["nan", "pattern"])
def test_guard_bands_detect_one_byte(dtype, poison):
    shape = (3, 5, 7, 3)  # 315 elements: not a multiple of anything
    view, chk = cr.guarded(shape, dtype, poison, device="cpu")
    assert tuple(view.shape) == shape and view.data_ptr() % 4096 == 0 and view.is_contiguous()
    if dtype != torch.uint8:
        assert torch.isnan(view.float()).all()  # the tensor itself starts as NaN
    chk()
    view.fill_(1)  # writing the tensor leaves the bands alone
    chk()
    lo, hi = chk.bands
    assert lo.numel() == hi.numel() == 4096
    assert lo.data_ptr() + 4096 == view.data_ptr() and hi.data_ptr() == view.data_ptr() + view.numel() * view.element_size()
    for band, at in ((hi, 0), (lo, 4095), (lo, 0), (hi, 4095)):
        old = int(band[at])
        band[at] = old ^ 1
        with pytest.raises(AssertionError, match="guard band"):
            chk()
        band[at] = old
        chk()


def test_guarded_fill_and_nan_bands():
    fill = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    view, chk = cr.guarded((2, 3, 4), torch.float32, "nan", device="cpu", fill=fill)
    assert torch.equal(view, fill)
    lo, hi = chk.bands
    assert torch.isnan(lo.view(torch.float32)).all() and torch.isnan(hi.view(torch.bfloat16).float()).all()
