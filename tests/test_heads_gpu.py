"""The fusion heads and the cross-entropy of csrc/head.hip against the float64 restatements of tests/head_ref.py, every element
within the bound DERIVED there (no tuned tolerance; tests/test_heads_cpu.py shows that the bounds hold for float32 in any
summation order and that a subtly wrong kernel lies at least 8 bounds outside, at these very shapes and routes).

In every case each output lies in a buffer with 64 sentinel values on either side, which must come back bit-unchanged, the
output itself starts as NaN (an element the kernel leaves out fails its bound), and a second identical call must give
bit-identical outputs.  The gated head is checked stage by stage: each stage's restatement starts from the device's own output
of the stage before (hx / hy, the two halves of ws), so every comparison is one sum deep."""
import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

PAD = 64


class Guard:
    """output buffers between sentinels"""

    def __init__(self):
        self.flat = []

    def new(self, *shape, dtype=torch.float32):
        numel = int(np.prod(shape))
        flat = torch.empty(numel + 2 * PAD, dtype=dtype, device=DEV)
        flat[PAD:PAD + numel] = float("nan") if dtype.is_floating_point else 0
        flat[:PAD] = self.pattern(dtype)
        flat[PAD + numel:] = self.pattern(dtype)
        self.flat.append((flat, numel))
        return flat[PAD:PAD + numel].view(*shape)

    @staticmethod
    def pattern(dtype):
        return (torch.arange(PAD, device=DEV) * 3 + 1000).to(dtype)

    def intact(self):
        for flat, numel in self.flat:
            want = self.pattern(flat.dtype)
            assert torch.equal(flat[:PAD], want) and torch.equal(flat[PAD + numel:], want), "a sentinel was overwritten"


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _twice(run):
    """run() -> ({name: tensor or None}, Guard), called twice: sentinels intact, outputs bit-identical.  -> {name: numpy}"""
    a, ga = run()
    b, gb = run()
    torch.cuda.synchronize()
    ga.intact()
    gb.intact()
    for k in a:
        if a[k] is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k + ": two identical calls differ"
    return {k: v.cpu().numpy() for k, v in a.items() if v is not None}


def _within(got, ref, keys, what):
    for k in keys:
        ex = R.excess(got[k], ref[k][0], ref[k][1])
        print(what, k, "excess", ex)
        assert ex <= 1.0, (what, k, "is", ex, "bounds from the float64 value")


def _devs(d):
    return {k: dev(v) for k, v in d.items()}


def _pick(d, has, key):
    return d[key] if has else None


# ------------------------------------------------------------------ concat / sum
@pytest.mark.parametrize("B,n", R.LIN_SHAPES)
@pytest.mark.parametrize("kind", ["concat", "sum"])
def test_lin_head(kind, B, n):
    """gdl_head_{concat,sum}_fwd with and without x_out / y_out, and gdl_head_{concat,sum}_bwd on every route of LIN_ROUTES."""
    d = R.lin_inputs(kind, B, n)
    D = _devs({k: v for k, v in d.items() if kind == "sum" or k not in ("Wx", "Wy", "bx", "by")})
    s = L.cur_stream()
    ref = R.lin_fwd(R.F64, kind, d["x"], d["y"], d["Wx"], d["bx"], d["Wy"], d["by"])
    for uni in (True, False):
        def fwd():
            g = Guard()
            o = dict(out=g.new(B, n), x_out=g.new(B, n) if uni else None, y_out=g.new(B, n) if uni else None)
            if kind == "concat":
                L.call("gdl_head_concat_fwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(D["W"]), L.ptr(D["b"]), L.ptr(o["out"]),
                       L.ptr(o["x_out"]), L.ptr(o["y_out"]), B, n, s)
            else:
                L.call("gdl_head_sum_fwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(D["Wx"]), L.ptr(D["bx"]), L.ptr(D["Wy"]), L.ptr(D["by"]),
                       L.ptr(o["out"]), L.ptr(o["x_out"]), L.ptr(o["y_out"]), B, n, s)
            return o, g

        got = _twice(fwd)
        _within(got, ref, ("out", "x_out", "y_out") if uni else ("out",), f"{kind} fwd")
    for route, (hx, hy, ho, reach, uni, wdx, wdw) in R.LIN_ROUTES.items():
        gx, gy, go = _pick(D, hx, "gx"), _pick(D, hy, "gy"), _pick(D, ho, "go")
        keys = R.lin_bwd_keys(kind, wdx, wdw)

        def bwd():
            g = Guard()
            o = dict(dx=g.new(B, R.HD) if wdx else None, dy=g.new(B, R.HD) if wdx else None)
            if kind == "concat":
                o.update(dW=g.new(n, 2 * R.HD) if wdw else None, db=g.new(n) if wdw else None)
                L.call("gdl_head_concat_bwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(D["W"]), L.ptr(gx), L.ptr(gy), L.ptr(go), reach, uni,
                       L.ptr(o["dx"]), L.ptr(o["dy"]), L.ptr(o["dW"]), L.ptr(o["db"]), B, n, s)
            else:
                for k, sh in (("dWx", (n, R.HD)), ("dbx", (n,)), ("dWy", (n, R.HD)), ("dby", (n,))):
                    o[k] = g.new(*sh) if wdw else None
                L.call("gdl_head_sum_bwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(D["Wx"]), L.ptr(D["Wy"]), L.ptr(gx), L.ptr(gy), L.ptr(go),
                       reach, uni, L.ptr(o["dx"]), L.ptr(o["dy"]), L.ptr(o["dWx"]), L.ptr(o["dbx"]), L.ptr(o["dWy"]), L.ptr(o["dby"]),
                       B, n, s)
            return o, g

        got = _twice(bwd)
        rb = R.lin_bwd(R.F64, kind, d["x"], d["y"], d["Wx"], d["Wy"], _pick(d, hx, "gx"), _pick(d, hy, "gy"), _pick(d, ho, "go"),
                       reach, uni)
        _within(got, rb, keys, f"{kind} bwd {route}")


# ------------------------------------------------------------------ gated
def _gated_shared_stages(d, got, wdx, wdw1, what):
    """dx / dy and dW1 .. db2 from the device's own dhx / dhy (the two halves of ws)"""
    B = d["x"].shape[0]
    dhx, dhy = got["ws"][:B * R.HD].reshape(B, R.HD), got["ws"][B * R.HD:].reshape(B, R.HD)
    if wdx:
        _within(got, R.gated_dx(R.F64, dhx, dhy, d["W1"], d["W2"]), ("dx", "dy"), what)
    if wdw1:
        _within(got, R.gated_dw1(R.F64, dhx, dhy, d["x"], d["y"]), ("dW1", "db1", "dW2", "db2"), what)
    return dhx, dhy


def _gated_grad_bufs(g, B, n, wdx, wdw1, wdwo):
    o = dict(ws=g.new(2 * B * R.HD), dx=g.new(B, R.HD) if wdx else None, dy=g.new(B, R.HD) if wdx else None)
    for k, sh in (("dW1", (R.HD, R.HD)), ("db1", (R.HD,)), ("dW2", (R.HD, R.HD)), ("db2", (R.HD,))):
        o[k] = g.new(*sh) if wdw1 else None
    o.update(dWo=g.new(n, R.HD) if wdwo else None, dbo=g.new(n) if wdwo else None)
    return o


@pytest.mark.parametrize("B,n", R.GATED_SHAPES)
def test_gated_dgl(B, n):
    """gdl_head_gated_fwd (with and without x_out / y_out) and gdl_head_gated_bwd: both phases of the DGL step and every optional
    output group."""
    d = R.gated_inputs(B, n)
    D = _devs(d)
    s = L.cur_stream()
    P = [L.ptr(D[k]) for k in ("W1", "b1", "W2", "b2", "Wo", "bo")]
    for uni in (True, False):
        def fwd():
            g = Guard()
            o = dict(hx=g.new(B, R.HD), hy=g.new(B, R.HD), out=g.new(B, n), x_out=g.new(B, n) if uni else None,
                     y_out=g.new(B, n) if uni else None)
            L.call("gdl_head_gated_fwd", L.ptr(D["x"]), L.ptr(D["y"]), *P, L.ptr(o["hx"]), L.ptr(o["hy"]), L.ptr(o["out"]),
                   L.ptr(o["x_out"]), L.ptr(o["y_out"]), B, n, s)
            return o, g

        f = _twice(fwd)
        _within(f, R.gated_hidden(R.F64, d["x"], d["y"], d["W1"], d["b1"], d["W2"], d["b2"]), ("hx", "hy"), "gated hidden")
        assert max(np.abs(f["hx"]).max(), np.abs(f["hy"]).max()) <= R.H_MAX
        _within(f, R.gated_logits(R.F64, f["hx"], f["hy"], d["Wo"], d["bo"]), ("out", "x_out", "y_out") if uni else ("out",),
                "gated logits")
    hx, hy = dev(f["hx"]), dev(f["hy"])
    for route, (hxg, hyg, hog, uni, wdx, wdw1, wdwo) in R.GATED_ROUTES.items():
        gx, gy, go = _pick(D, hxg, "gx"), _pick(D, hyg, "gy"), _pick(D, hog, "go")

        def bwd():
            g = Guard()
            o = _gated_grad_bufs(g, B, n, wdx, wdw1, wdwo)
            L.call("gdl_head_gated_bwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(hx), L.ptr(hy), L.ptr(D["W1"]), L.ptr(D["W2"]), L.ptr(D["Wo"]),
                   L.ptr(gx), L.ptr(gy), L.ptr(go), uni, L.ptr(o["dx"]), L.ptr(o["dy"]), L.ptr(o["dW1"]), L.ptr(o["db1"]), L.ptr(o["dW2"]),
                   L.ptr(o["db2"]), L.ptr(o["dWo"]), L.ptr(o["dbo"]), L.ptr(o["ws"]), B, n, s)
            return o, g

        got = _twice(bwd)
        what = f"gated bwd {route}"
        if wdx or wdw1:
            rd = R.gated_dh(R.F64, f["hx"], f["hy"], d["Wo"], _pick(d, hxg, "gx"), _pick(d, hyg, "gy"))
            ex = R.excess(got["ws"], np.concatenate([rd["dhx"][0].ravel(), rd["dhy"][0].ravel()]),
                          np.concatenate([rd["dhx"][1].ravel(), rd["dhy"][1].ravel()]))
            print(what, "dh excess", ex)
            assert ex <= 1.0, (what, "dh", ex)
            _gated_shared_stages(d, got, wdx, wdw1, what)
        else:
            assert np.isnan(got["ws"]).all()  # (no stage that writes ws was asked for)
        if wdwo:
            _within(got, R.gated_dwo(R.F64, f["hx"], f["hy"], _pick(d, hxg, "gx"), _pick(d, hyg, "gy"), _pick(d, hog, "go"), uni),
                    ("dWo", "dbo"), what)


@pytest.mark.parametrize("x_gate", [1, 0])
@pytest.mark.parametrize("B,n", R.GATED_SHAPES)
def test_gated_joint(B, n, x_gate):
    """gdl_head_gated_joint_fwd / _bwd with either gate and every optional output group."""
    d = R.gated_inputs(B, n)
    D = _devs(d)
    s = L.cur_stream()
    P = [L.ptr(D[k]) for k in ("W1", "b1", "W2", "b2", "Wo", "bo")]

    def fwd():
        g = Guard()
        o = dict(hx=g.new(B, R.HD), hy=g.new(B, R.HD), out=g.new(B, n))
        L.call("gdl_head_gated_joint_fwd", L.ptr(D["x"]), L.ptr(D["y"]), *P, L.ptr(o["hx"]), L.ptr(o["hy"]), L.ptr(o["out"]), x_gate, B, n, s)
        return o, g

    f = _twice(fwd)
    _within(f, R.gated_hidden(R.F64, d["x"], d["y"], d["W1"], d["b1"], d["W2"], d["b2"]), ("hx", "hy"), "gated hidden")
    _within(f, R.gated_joint_logits(R.F64, f["hx"], f["hy"], d["Wo"], d["bo"], x_gate), ("out",), "gated joint logits")
    hx, hy = dev(f["hx"]), dev(f["hy"])
    for route, (wdx, wdw1, wdwo) in R.GATED_JOINT_ROUTES.items():
        def bwd():
            g = Guard()
            o = _gated_grad_bufs(g, B, n, wdx, wdw1, wdwo)
            L.call("gdl_head_gated_joint_bwd", L.ptr(D["x"]), L.ptr(D["y"]), L.ptr(hx), L.ptr(hy), L.ptr(D["W1"]), L.ptr(D["W2"]),
                   L.ptr(D["Wo"]), L.ptr(D["go"]), x_gate, L.ptr(o["dx"]), L.ptr(o["dy"]), L.ptr(o["dW1"]), L.ptr(o["db1"]), L.ptr(o["dW2"]),
                   L.ptr(o["db2"]), L.ptr(o["dWo"]), L.ptr(o["dbo"]), L.ptr(o["ws"]), B, n, s)
            return o, g

        got = _twice(bwd)
        what = f"gated joint bwd {route}"
        if wdx or wdw1:
            rd = R.gated_joint_dh(R.F64, f["hx"], f["hy"], d["Wo"], d["go"], x_gate)
            ex = R.excess(got["ws"], np.concatenate([rd["dhx"][0].ravel(), rd["dhy"][0].ravel()]),
                          np.concatenate([rd["dhx"][1].ravel(), rd["dhy"][1].ravel()]))
            print(what, "dh excess", ex)
            assert ex <= 1.0, (what, "dh", ex)
            _gated_shared_stages(d, got, wdx, wdw1, what)
        else:
            assert np.isnan(got["ws"]).all()
        if wdwo:
            gate, val = (f["hx"], f["hy"]) if x_gate else (f["hy"], f["hx"])
            _within(got, R.gated_dwo(R.F64, gate, val, None, None, d["go"], 0), ("dWo", "dbo"), what)


# ------------------------------------------------------------------ softmax cross-entropy
def _ce(lg, lab, scale, with_d=True):
    B, n = lg.shape

    def run():
        g = Guard()
        o = dict(loss=g.new(1), dlogits=g.new(B, n) if with_d else None)
        L.call("gdl_softmax_ce", L.ptr(lg), L.ptr(lab), scale, L.ptr(o["loss"]), L.ptr(o["dlogits"]), B, n, L.cur_stream())
        return o, g

    return _twice(run)


def _ce3(lgs, lab, scales, with_d=(True, True, True)):
    B, n = lgs[0].shape

    def run():
        g = Guard()
        o = dict(loss=g.new(3))
        for k in range(3):
            o[f"d{k}"] = g.new(B, n) if with_d[k] else None
        L.call("gdl_softmax_ce3", L.ptr(lgs[0]), L.ptr(lgs[1]), L.ptr(lgs[2]), L.ptr(lab), *scales, L.ptr(o["loss"]), L.ptr(o["d0"]),
               L.ptr(o["d1"]), L.ptr(o["d2"]), B, n, L.cur_stream())
        return o, g

    return _twice(run)


@pytest.mark.parametrize("B,n", R.CE_SHAPES)
def test_softmax_ce(B, n):
    """gdl_softmax_ce and gdl_softmax_ce3 on the dispatch edges (thread form / wave form on 16 and 8 waves / thread form; the
    256 loss slots), labels 0 and n - 1, a row of equal logits and one with a spread of 160; NULL dlogits leaves the loss's bits."""
    lgs, lab = R.ce3_inputs(B, n)
    lgd, labd = [dev(lg) for lg in lgs], torch.from_numpy(lab).to(DEV)
    ref = R.softmax_ce(R.F64, lgs[0], lab, R.CE_SCALE)
    got = _ce(lgd[0], labd, R.CE_SCALE)
    _within(got, ref, ("loss", "dlogits"), "softmax_ce")
    alone = _ce(lgd[0], labd, R.CE_SCALE, with_d=False)
    assert alone["loss"].tobytes() == got["loss"].tobytes()
    refs = [R.softmax_ce(R.F64, lg, lab, sc) for lg, sc in zip(lgs, R.CE3_SCALES)]
    got3 = _ce3(lgd, labd, R.CE3_SCALES)
    some = _ce3(lgd, labd, R.CE3_SCALES, with_d=(False, True, False))
    assert some["loss"].tobytes() == got3["loss"].tobytes() and some["d1"].tobytes() == got3["d1"].tobytes()
    for k in range(3):
        ex = R.excess(got3["loss"][k], refs[k]["loss"][0], refs[k]["loss"][1])
        exd = R.excess(got3[f"d{k}"], refs[k]["dlogits"][0], refs[k]["dlogits"][1])
        print("softmax_ce3 set", k, "loss excess", ex, "dlogits excess", exd)
        assert ex <= 1.0 and exd <= 1.0, ("softmax_ce3 set", k, ex, exd)


@pytest.mark.parametrize("bad", [-1, "n"])
@pytest.mark.parametrize("B,n", [(7, 6), (7, 309)])
def test_softmax_ce_invalid_label(B, n, bad):
    """One label outside [0, n), in the thread form and in the wave form (softmax_ce_block compares such a label and never indexes
    with it): the loss is NaN, that row's dlogits is the softmax term alone, every other row is within its bound."""
    lgs, lab = R.ce3_inputs(B, n)
    lab = lab.copy()
    lab[3] = n if bad == "n" else bad
    lgd, labd = [dev(lg) for lg in lgs], torch.from_numpy(lab).to(DEV)
    ref = R.softmax_ce(R.F64, lgs[0], lab, R.CE_SCALE)  # (its row 3 has no one-hot term: tests/test_heads_cpu.py)
    got = _ce(lgd[0], labd, R.CE_SCALE)
    assert np.isnan(got["loss"]).all()
    _within(got, ref, ("dlogits",), "softmax_ce, invalid label")
    got3 = _ce3(lgd, labd, R.CE3_SCALES)
    assert np.isnan(got3["loss"]).all()
    for k in range(3):
        r = R.softmax_ce(R.F64, lgs[k], lab, R.CE3_SCALES[k])
        assert R.excess(got3[f"d{k}"], r["dlogits"][0], r["dlogits"][1]) <= 1.0, k


# ------------------------------------------------------------------ gdl_head_uni_dfeat's refusal, gdl_eval_count
def test_head_uni_dfeat_refuses_513_classes():
    """More classes than the body stages in LDS (HB_MAXN = 512): an error and no launch -- df keeps its bits."""
    B, n = 3, 513
    d = R.lin_inputs("concat", 5, 512)
    x = dev(d["x"][:B])
    W = dev(np.concatenate([d["W"], d["W"][:1]]))
    b = dev(np.concatenate([d["b"], d["b"][:1]]))
    lab = torch.zeros(B, dtype=torch.int64, device=DEV)
    g = Guard()
    df = g.new(B, R.HD)
    df.copy_(torch.arange(B * R.HD, device=DEV).view(B, R.HD))
    before = df.clone()
    with pytest.raises(L.GdlError, match="512"):
        L.call("gdl_head_uni_dfeat", L.ptr(x), L.ptr(W), 1024, L.ptr(b), L.ptr(lab), 4.0, L.ptr(df), B, n, L.cur_stream())
    torch.cuda.synchronize()
    g.intact()
    assert torch.equal(_bits(df), _bits(before))


def _valid_counts(outs, labels, n):
    """num[label]++, acc_h[label] += (first arg-max of set h == label), over the samples whose label is a class"""
    cnt = np.zeros((4, n), dtype=np.int64)
    for i, lab in enumerate(labels):
        if not 0 <= lab < n:
            continue
        cnt[0, lab] += 1
        for h, o in enumerate(outs):
            if o is not None and int(np.argmax(o[i])) == lab:
                cnt[1 + h, lab] += 1
    return cnt


def _eval_count(outs, labels, n, uni=True):
    B = len(labels)
    d = [dev(o) if o is not None else None for o in outs]
    lab = torch.from_numpy(labels).to(DEV)

    def run():
        g = Guard()
        o = dict(num=g.new(n, dtype=torch.int64), acc=g.new(n, dtype=torch.int64),
                 acc_a=g.new(n, dtype=torch.int64) if uni else None, acc_v=g.new(n, dtype=torch.int64) if uni else None)
        L.call("gdl_eval_count", L.ptr(d[0]), L.ptr(d[1]) if uni else None, L.ptr(d[2]) if uni else None, L.ptr(lab), B, n,
               L.ptr(o["num"]), L.ptr(o["acc"]), L.ptr(o["acc_a"]), L.ptr(o["acc_v"]), L.cur_stream())
        return o, g

    return _twice(run)


@pytest.mark.parametrize("uni", [True, False])
@pytest.mark.parametrize("B", [1, 40])
def test_eval_count_edges(B, uni):
    """gdl_eval_count at one sample, and with out_a / out_v and their counters NULL."""
    n = 6
    rs = np.random.default_rng([3, B])
    outs = [np.round(rs.standard_normal((B, n)).astype(np.float32) * 2, 1) for _ in range(3)]
    labels = rs.integers(0, n, B).astype(np.int64)
    got = _eval_count(outs, labels, n, uni)
    want = _valid_counts(outs if uni else [outs[0], None, None], labels, n)
    for k, name in enumerate(("num", "acc", "acc_a", "acc_v")):
        if name in got:
            np.testing.assert_array_equal(got[name], want[k], err_msg=name)


def test_eval_count_skips_labels_that_are_no_class():
    """Labels -1, n, 2^31 + 1 and 2^32 + 1 among valid ones: all four samples are skipped and change no counter.  (The label is
    range-checked as the 64-bit value it is; narrowed first, 2^32 + 1 would count as class 1.  None of the four can index memory:
    the kernel returns before it uses the label.)"""
    B, n = 24, 6
    rs = np.random.default_rng(11)
    outs = [np.round(rs.standard_normal((B, n)).astype(np.float32) * 2, 1) for _ in range(3)]
    labels = rs.integers(0, n, B).astype(np.int64)
    bad = {2: -1, 7: n, 13: 2 ** 31 + 1, 20: 2 ** 32 + 1}
    for i, v in bad.items():
        labels[i] = v
        for o in outs:
            o[i, 1] = 9.0  # the arg-max of these rows is class 1: what 2^32 + 1 narrows to
    got = _eval_count(outs, labels, n)
    want = _valid_counts(outs, labels, n)
    assert want[0].sum() == B - len(bad)
    for k, name in enumerate(("num", "acc", "acc_a", "acc_v")):
        np.testing.assert_array_equal(got[name], want[k], err_msg=name)
