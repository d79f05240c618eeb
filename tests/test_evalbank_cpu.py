"""CPU-only checks of the evaluation report's score bank (csrc/evalbank.hip, gdl/evaluate.py): the NumPy restatement
(tests/evalbank_ref.py) against scikit-learn's recorded and live average precision and against itself, the C ABI's presence,
its size queries and every host-side refusal (no launch, no GPU), and ScoreBank's refusal of a CPU device."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "iccv2025-gdl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import evalbank_ref as er  # noqa: E402
from gdl import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "evalbank_small.npz")
CASES = ("a", "b", "c")


def sklearn_bound(N):
    """scikit-learn's own float64 evaluation, -sum_k (R_k - R_{k-1}) P_k over at most N thresholds: two rounded recalls and
    their difference (3 x 2^-53 absolute, all values <= 1), times a rounded precision, added in float64 -- 4 roundings a term
    plus N for the sum, first order."""
    return (5 * N + 2) * er.U64


def restated_ap(lg, lab):
    n = lg.shape[1]
    r = er.restate([lg], lab, n)
    p32 = r["probs"][0].astype(np.float32)
    ap, npos = er.ap_exact(p32, r["labels"])
    return r, p32, ap, npos


def test_restatement_meets_recorded_sklearn():
    g = np.load(GOLDEN)
    for name in CASES:
        lg, lab, want = g[name + ".logits"], g[name + ".labels"], g[name + ".ap"]
        assert lg.dtype == np.float32 and lab.dtype == np.int64
        _, _, ap, npos = restated_ap(lg, lab)
        assert all(k > 0 for k in npos)
        for c, (a, w) in enumerate(zip(ap, want)):
            assert abs(Fraction(float(w)) - a) <= sklearn_bound(lg.shape[0]), (name, c, float(a), w)


def test_restatement_meets_live_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    for kind in er.SCORE_KINDS:
        for N, n in ((1, 1), (40, 3), (257, 6)):
            lg, lab = er.make_logits(kind, N, n, 0), er.make_labels(N, n, 0)
            _, p32, ap, npos = restated_ap(lg, lab)
            for c in range(n):
                if npos[c] == 0:
                    assert ap[c] is None
                    continue
                got = metrics.average_precision_score((lab == c).astype(int), p32[c])
                assert abs(Fraction(float(got)) - ap[c]) <= sklearn_bound(N), (kind, N, n, c)


def test_restatement_top1_is_its_argmax_count():
    for kind in er.SCORE_KINDS:
        N, n = 200, 7
        sets = [er.make_logits(kind, N, n, s) for s in range(3)]
        lab = er.make_labels(N, n, 1)
        lab[[3, 50]] = [-1, n]
        sets[1][7, 2] = np.nan
        r = er.restate(sets, lab, n)
        assert r["skipped"] == 2 and list(r["nonfinite"]) == [0, 1, 0]
        ok = r["labels"] >= 0
        for s in range(3):
            fin = np.isfinite(sets[s]).all(axis=1)
            use = ok & fin
            right = int((np.argmax(sets[s][use], axis=1) == r["labels"][use]).sum())
            assert r["rank_hist"][s, 0] == right == int(np.trace(r["confusion"][s]))
            assert er.topk(r["rank_hist"], 1)[s] == Fraction(right, int(use.sum()))
            assert er.topk(r["rank_hist"], n)[s] == 1
            assert r["confusion"][s].sum() == r["rank_hist"][s].sum() == int(use.sum())
            assert ((r["rank"][s] == 0) == (r["pred"][s] == r["labels"]))[use].all()
        assert (r["num"] == np.bincount(r["labels"][ok], minlength=n)).all()


def test_probability_bound_holds_for_float32_softmax():
    """The bound is not vacuous and not wrong on the host: a float32 evaluation of the same lines, ascending sums, lies inside
    it; probabilities off by one part in a thousand lie far outside."""
    for kind in er.SCORE_KINDS:
        lg = er.make_logits(kind, 33, 65, 2)
        p, b = er.softmax_bound(lg)
        mx = lg.max(axis=1, keepdims=True)
        e = np.exp(lg - mx)
        se = np.zeros((33, 1), np.float32)
        for j in range(65):
            se[:, 0] += e[:, j]
        p32 = np.exp(lg - (mx + np.log(se)))
        assert p32.dtype == np.float32
        assert (np.abs(p32 - p) <= b).all()
        big = p > 1e-3
        assert (np.abs(p * 1.001 - p)[big] > 8 * b[big]).all()


def test_abi_presence_and_size_queries():
    lib = L.load()
    want = {"gdl_eval_bank_bytes": 3, "gdl_eval_bank_reset_bytes": 2, "gdl_eval_bank_append": 12, "gdl_eval_bank_ap": 7}
    for name, nargs in want.items():
        assert name in L.SIGNATURES and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.gdl_eval_bank_append.restype is ctypes.c_int and lib.gdl_eval_bank_bytes.restype is ctypes.c_size_t
    B = lib.gdl_eval_bank_bytes
    # monotone in each argument
    assert 0 < B(6, 100, 1) < B(7, 100, 1) < B(7, 101, 1) < B(7, 101, 3)
    assert B(6, 100, 1) < B(6, 100, 3) and B(6, 100, 3) < B(6, 164, 3) and B(309, 100, 3) < B(512, 100, 3)
    # holds what the header lists
    for n, cap, S in ((6, 100, 1), (309, 15360, 3), (512, 1, 3)):
        rb = lib.gdl_eval_bank_reset_bytes(n, S)
        assert rb == 32 + 8 * n * (1 + S + S * n)
        assert B(n, cap, S) >= rb + 8 * S * n + 24 + 4 * cap + 4 * S * n * cap
    for bad in ((0, 10, 1), (513, 10, 1), (6, 0, 1), (6, 10, 2), (6, 10, 0), (6, 1 << 31, 1)):
        assert B(*bad) == 0
    assert lib.gdl_eval_bank_reset_bytes(513, 1) == 0 and lib.gdl_eval_bank_reset_bytes(6, 2) == 0


def test_every_bad_argument_is_refused_on_the_host():
    lib = L.load()
    one = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    n, cap = 6, 100
    big = lib.gdl_eval_bank_bytes(512, 1 << 20, 3)

    def append(bank=one, nbytes=big, n=n, cap=cap, sets=3, out=one, oa=one, ov=one, lab=one, B=4, off=0):
        rc = lib.gdl_eval_bank_append(bank, nbytes, n, cap, sets, out, oa, ov, lab, B, off, None)
        return rc, lib.gdl_last_error()

    def ap(bank=one, nbytes=big, n=n, cap=cap, sets=3, N=10):
        rc = lib.gdl_eval_bank_ap(bank, nbytes, n, cap, sets, N, None)
        return rc, lib.gdl_last_error()

    for call in (append, ap):
        for kw, word in ((dict(bank=None), b"null bank"), (dict(n=513), b"n_classes"), (dict(n=0), b"n_classes"),
                         (dict(sets=2), b"sets must be"), (dict(cap=0), b"capacity"),
                         (dict(nbytes=lib.gdl_eval_bank_bytes(n, cap, 3) - 1), b"gdl_eval_bank_bytes"),
                         (dict(bank=ctypes.c_void_p(264)), b"16-byte aligned")):
            rc, msg = call(**kw)
            assert rc != 0 and word in msg and msg.startswith(b"eval_bank_"), (call.__name__, kw, msg)
    for kw, word in ((dict(out=None), b"null out or labels"), (dict(lab=None), b"null out or labels"),
                     (dict(sets=1), b"sets = 1"), (dict(sets=1, oa=None), b"sets = 1"), (dict(oa=None), b"needs out_a and out_v"),
                     (dict(ov=None), b"needs out_a and out_v"), (dict(B=0), b"B must be"), (dict(off=-1), b"do not fit"),
                     (dict(off=cap - 3), b"do not fit"), (dict(B=cap + 1), b"do not fit")):
        rc, msg = append(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    for N in (-1, cap + 1):
        rc, msg = ap(N=N)
        assert rc != 0 and b"samples in a bank" in msg


def test_score_bank_refuses_a_cpu_device():
    import gdl

    with pytest.raises(L.GdlError, match="cuda"):
        gdl.ScoreBank(6, 100, sets=3, device="cpu")
    from gdl.evaluate import ScoreBank

    assert gdl.ScoreBank is ScoreBank
