"""The bounds of tests/head_ref.py, without a GPU, on every shape and route tests/test_heads_gpu.py uses:
  * the float32 evaluation of each restatement, with every sum an explicit chain in ascending and in descending index order,
    lies within the bound of the float64 value (the bounds hold for a correct float32 kernel in any summation order);
  * each mutation of MUTATIONS -- a subtly wrong kernel -- moves at least one output of its entry point by at least 8 bounds,
    wherever the mutation can show at all (the rules are spelled out next to each use).
The staged gated restatements take, as on the device, the float32 rounding of the stage before as their input."""
import numpy as np
import pytest

import head_ref as R

ORDERS = (+1, -1)
FACTOR = 8.0


def _inside(fn, args, kw=None, keys=None):
    """float32 in both orders within the float64 bounds; returns the float64 result {name: (value, bound)}"""
    kw = kw or {}
    ref = fn(R.F64, *args, **kw)
    for o in ORDERS:
        got = fn(R.F32(o), *args, **kw)
        for k in keys or ref:
            ex = R.excess(got[k][0], ref[k][0], ref[k][1])
            assert ex <= 1.0, (fn.__name__, k, "order", o, "excess", ex)
    return ref


def _outside(fn, args, ref, muts, kw=None, keys=None):
    """every mutation in `muts` at least FACTOR bounds outside on at least one of the outputs `keys`"""
    kw = kw or {}
    for m in muts:
        assert m in R.MUTATIONS[fn.__name__], m
        bad = fn(R.F64, *args, mut=m, **kw)
        worst = max(R.excess(bad[k][0], ref[k][0], ref[k][1]) for k in (keys or ref))
        assert worst >= FACTOR, (fn.__name__, m, "only", worst, "bounds outside")


def _pick(d, has, key):
    return d[key] if has else None


# ------------------------------------------------------------------ concat / sum
@pytest.mark.parametrize("B,n", R.LIN_SHAPES)
@pytest.mark.parametrize("kind", ["concat", "sum"])
def test_lin_fwd(kind, B, n):
    d = R.lin_inputs(kind, B, n)
    args = (kind, d["x"], d["y"], d["Wx"], d["bx"], d["Wy"], d["by"])
    ref = _inside(R.lin_fwd, args)
    _outside(R.lin_fwd, args, ref, ("feat511", "bias") + (("bx_for_sum",) if kind == "sum" else ()))
    # without x_out / y_out (the NULL variant) the mutations must show on `out` alone
    _outside(R.lin_fwd, args, ref, ("feat511", "bias") + (("bx_for_sum",) if kind == "sum" else ()), keys=("out",))


@pytest.mark.parametrize("route", list(R.LIN_ROUTES))
@pytest.mark.parametrize("B,n", R.LIN_SHAPES)
@pytest.mark.parametrize("kind", ["concat", "sum"])
def test_lin_bwd(kind, B, n, route):
    hx, hy, ho, reach, uni, wdx, wdw = R.LIN_ROUTES[route]
    d = R.lin_inputs(kind, B, n)
    args = (kind, d["x"], d["y"], d["Wx"], d["Wy"], _pick(d, hx, "gx"), _pick(d, hy, "gy"), _pick(d, ho, "go"), reach, uni)
    keys = R.lin_bwd_keys(kind, wdx, wdw)
    ref = _inside(R.lin_bwd, args, keys=keys)
    muts = []
    if wdx and (hx or hy or (reach and ho)):
        muts.append("class")  # dx / dy are the sums over the classes
    if wdw and (ho or (uni and (hx or hy))):
        muts.append("sample")  # dW / db are the sums over the samples
    if (hx or hy) and (wdx or (uni and wdw)):
        muts.append("swap")
    if ho and wdx:
        muts.append("reach")  # out_reaches_xy decides whether g_out reaches dx / dy
    if (hx or hy) and wdw:
        muts.append("uni")  # uni_in_dw decides whether the unimodal gradients reach dW / db
    _outside(R.lin_bwd, args, ref, muts, keys=keys)


# ------------------------------------------------------------------ gated
def _f32(v):
    return np.asarray(v[0], dtype=np.float32)


@pytest.mark.parametrize("B,n", R.GATED_SHAPES)
def test_gated_stages(B, n):
    d = R.gated_inputs(B, n)
    a = (d["x"], d["y"], d["W1"], d["b1"], d["W2"], d["b2"])
    h = _inside(R.gated_hidden, a)
    _outside(R.gated_hidden, a, h, ("feat511", "bias"))
    hx, hy = _f32(h["hx"]), _f32(h["hy"])
    assert max(np.abs(hx).max(), np.abs(hy).max()) <= R.H_MAX  # the input range the transcendental allowance assumes
    # the DGL form
    a = (hx, hy, d["Wo"], d["bo"])
    ref = _inside(R.gated_logits, a)
    _outside(R.gated_logits, a, ref, ("feat511", "bias"))
    _outside(R.gated_logits, a, ref, ("feat511", "bias"), keys=("out",))
    a = (hx, hy, d["Wo"], d["gx"], d["gy"])
    dh = _inside(R.gated_dh, a)
    _outside(R.gated_dh, a, dh, ("class", "swap", "act"))
    dhs = [(_f32(dh["dhx"]), _f32(dh["dhy"]))]
    for hxg, hyg, hog, uni in sorted({r[:4] for r in R.GATED_ROUTES.values()}):
        a = (hx, hy, _pick(d, hxg, "gx"), _pick(d, hyg, "gy"), _pick(d, hog, "go"), uni)
        ref = _inside(R.gated_dwo, a)
        # "sample" shows when any gradient reaches dWo; "swap" and "uni" when the unimodal ones are given (and, for swap, used)
        muts = ["sample"] + (["uni"] if (hxg or hyg) else []) + (["swap"] if uni and (hxg or hyg) else [])
        _outside(R.gated_dwo, a, ref, muts)
    # the joint form, either gate
    for x_gate in (1, 0):
        a = (hx, hy, d["Wo"], d["bo"], x_gate)
        ref = _inside(R.gated_joint_logits, a)
        _outside(R.gated_joint_logits, a, ref, ("feat511", "bias"))
        a = (hx, hy, d["Wo"], d["go"], x_gate)
        dh = _inside(R.gated_joint_dh, a)
        _outside(R.gated_joint_dh, a, dh, ("class", "act"))
        dhs.append((_f32(dh["dhx"]), _f32(dh["dhy"])))
        gate, val = (hx, hy) if x_gate else (hy, hx)
        a = (gate, val, None, None, d["go"], 0)
        ref = _inside(R.gated_dwo, a)
        _outside(R.gated_dwo, a, ref, ("sample",))
    # the stages both forms share, from each form's dhx / dhy
    for dhx, dhy in dhs:
        a = (dhx, dhy, d["W1"], d["W2"])
        ref = _inside(R.gated_dx, a)
        _outside(R.gated_dx, a, ref, ("feat511",))
        a = (dhx, dhy, d["x"], d["y"])
        ref = _inside(R.gated_dw1, a)
        _outside(R.gated_dw1, a, ref, ("sample",))


# ------------------------------------------------------------------ softmax cross-entropy
@pytest.mark.parametrize("B,n", R.CE_SHAPES)
def test_softmax_ce(B, n):
    lab = R.ce_inputs(B, n)[1]
    assert lab.min() == (0 if B >= 2 else n - 1) and lab.max() == n - 1
    for a in R.ce_cases(B, n):
        ref = _inside(R.softmax_ce, a)
        # with one class every loss term and every dlogits element is zero: leaving a sample out or dividing by B - 1 changes
        # nothing there; leaving the class out of the sum of exponentials and dropping the one-hot term still do
        _outside(R.softmax_ce, a, ref, ("class", "onehot") + (("sample", "bm1") if n > 1 else ()))
        _outside(R.softmax_ce, a, ref, ("class",) + (("sample", "bm1") if n > 1 else ()), keys=("loss",))  # NULL dlogits


@pytest.mark.parametrize("bad", [-1, "n"])
@pytest.mark.parametrize("B,n", [(7, 6), (7, 309)])
def test_softmax_ce_invalid_label(B, n, bad):
    """The restatement's rule for a label outside [0, n): NaN loss, that row's dlogits the softmax term alone, other rows as
    with the valid label."""
    lg, lab = R.ce_inputs(B, n)
    ref = R.softmax_ce(R.F64, lg, lab, 4.0)
    lab2 = lab.copy()
    lab2[3] = n if bad == "n" else bad
    got = R.softmax_ce(R.F64, lg, lab2, 4.0)
    assert np.isnan(got["loss"][0])
    keep = np.arange(B) != 3
    np.testing.assert_array_equal(got["dlogits"][0][keep], ref["dlogits"][0][keep])
    p = np.exp(lg[3].astype(np.float64) - lg[3].max())
    np.testing.assert_allclose(got["dlogits"][0][3], 4.0 * p / p.sum() / B, rtol=1e-12)
    for o in ORDERS:
        g32 = R.softmax_ce(R.F32(o), lg, lab2, 4.0)
        assert np.isnan(g32["loss"][0])
        assert R.excess(g32["dlogits"][0], got["dlogits"][0], got["dlogits"][1]) <= 1.0
