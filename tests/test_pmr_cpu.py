"""CPU-only checks of what the GPU tests of prototypical modal rebalance are measured against (tests/pmr_ref.py): the float64
restatement against torch float64 autograd of the literal form sqrt(dot(x - p, x - p)) -> -d -> CrossEntropyLoss, the update rule
against a plain Python loop, the float32 mirrors (the fold, the fused multiply-add) against exact arithmetic -- and the argument
checks of gdl.Prototypes and DGLTrainer(prototypes=...) that need no GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pmr_ref as pref  # noqa: E402
from gdl import _lib as L  # noqa: E402


def _case(seed, B, n, scale=1.0):
    r = np.random.default_rng([41, seed])
    f = (0.5 * scale * np.abs(r.standard_normal((B, 512)))).astype(np.float32)
    P = (0.5 * scale * np.abs(r.standard_normal((n, 512)))).astype(np.float32)
    return f, P, r.integers(0, n, B)


def _torch_literal(f, P, labels):
    """The published form, transcribed: a double loop of sqrt(dot(x - p, x - p)), the negated distances as logits,
    CrossEntropyLoss; float64 autograd for d lossp / d f."""
    x = torch.from_numpy(f.astype(np.float64)).requires_grad_(True)
    p = torch.from_numpy(P.astype(np.float64))
    rows = []
    for i in range(x.shape[0]):
        rows.append(torch.stack([torch.sqrt(torch.dot(x[i] - p[j], x[i] - p[j])) for j in range(p.shape[0])]))
    sim = -torch.stack(rows)
    loss = torch.nn.CrossEntropyLoss()(sim, torch.from_numpy(np.asarray(labels, dtype=np.int64)))
    loss.backward()
    score = sum(torch.softmax(sim, dim=1)[i][labels[i]] for i in range(x.shape[0]))
    return sim.detach().numpy(), float(loss.detach()), x.grad.numpy(), float(score.detach())


@pytest.mark.parametrize("B,n,scale", [(1, 1, 1.0), (3, 6, 1.0), (5, 17, 1.0), (4, 33, 8.0)])
def test_restatement_against_torch_autograd(B, n, scale):
    f, P, labels = _case(B * 100 + n, B, n, scale)
    r = pref.proto_ce(f, P, labels)
    sim, loss, grad, score = _torch_literal(f, P, labels)
    np.testing.assert_allclose(r["sim"], sim, rtol=1e-13, atol=0)
    np.testing.assert_allclose(r["lossp"], loss, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["score"], score, rtol=1e-12)
    np.testing.assert_allclose(r["u"], grad, rtol=1e-10, atol=1e-15 * max(1.0, np.abs(grad).max()))
    assert r["sim"].shape == (B, n) and r["u"].shape == (B, 512)
    if scale == 1.0 and n > 1:
        assert 5 < r["d"].mean() < 15  # the magnitudes the GPU bounds are quoted at


def test_restatement_conventions():
    """A zero distance gives q = 0 and a finite u (torch: NaN); a label outside [0, n) gives no one-hot term, a score term of 0
    and a NaN loss term."""
    f, P, labels = _case(7, 4, 6)
    f[1] = P[2]
    labels = np.array([0, 2, 6, -1])
    r = pref.proto_ce(f, P, labels)
    assert r["d"][1, 2] == 0 and r["q"][1, 2] == 0 and np.isfinite(r["u"]).all()
    assert r["term_p"][2] == 0 and r["term_p"][3] == 0 and np.isnan(r["term_l"][2:]).all() and np.isfinite(r["term_l"][:2]).all()
    assert np.isnan(r["lossp"])
    np.testing.assert_allclose(r["q"][2] * r["d"][2] * 4, r["p"][2], rtol=1e-12)  # no one-hot term in the row
    *_, grad, _ = _torch_literal(f, P, np.array([0, 2, 0, 0]))
    assert np.isnan(grad[1]).all()  # the departure: torch's sqrt backward at zero
    b = pref.proto_ce_bounds(r, 4)
    assert all(np.isfinite(v).all() and (v > 0).all() for v in b.values())


def test_coefficient_rule():
    assert pref.coefficients(2.0, 1.0, 0.7) == (2.0, 0.0, 0.7)
    assert pref.coefficients(1.0, 2.0, 0.7) == (0.5, 0.7, 0.0)
    assert pref.coefficients(1.5, 1.5, 0.7) == (1.0, 0.0, 0.0)
    rho, beta, lam = pref.coefficients(np.float32(1.0), np.float32(0.0), 0.7)
    assert np.isinf(rho) and beta == 0 and lam == np.float32(0.7) and lam.dtype == np.float32
    rho, beta, lam = pref.coefficients(np.float32(0.0), np.float32(0.0), 0.7)
    assert np.isnan(rho) and beta == 0 and lam == 0
    rho, beta, lam = pref.coefficients(np.float32("nan"), np.float32(1.0), 0.7)
    assert np.isnan(rho) and beta == 0 and lam == 0


def test_fold_and_stats_mirror():
    """fold256 adds in the stated order (checked against an index-by-index loop); apply_stats puts the pieces where
    gdl_proto_apply's stats[8] has them."""
    r = np.random.default_rng(5)
    for B in (1, 3, 64, 300, 700):
        v = r.random(B).astype(np.float32)
        p = [np.float32(0)] * 256
        for i in range(B):
            p[i & 255] = np.float32(p[i & 255] + v[i])
        o = 128
        while o:
            for i in range(o):
                p[i] = np.float32(p[i] + p[i + o])
            o >>= 1
        assert pref.fold256(v) == p[0]
    ta, tv = r.random((2, 300)).astype(np.float32), r.random((2, 300)).astype(np.float32) * np.float32(0.5)
    s = pref.apply_stats(ta, tv, 0.9)
    assert s.dtype == np.float32 and s[0] == pref.fold256(ta[0]) and s[1] == pref.fold256(tv[0]) and s[2] == s[0] / s[1]
    assert s[2] > 1 and s[3] == 0 and s[4] == np.float32(0.9) and s[5] == pref.fold256(ta[1]) / np.float32(300) and s[7] == 0


def test_fmaf32_is_correctly_rounded():
    """against exact rational arithmetic, on random operands and on sums built to sit near a float32 rounding tie (where
    rounding the float64 sum first would round twice)"""
    r = np.random.default_rng(11)
    a = r.standard_normal(400).astype(np.float32)
    b = r.standard_normal(400).astype(np.float32)
    c = (r.standard_normal(400) * 10.0 ** r.integers(-6, 3, 400)).astype(np.float32)
    # near a tie of the float32 rounding: a b = 2^-24 (half an ulp of 1) + 2^-46, exactly 2^-24, and 2^-24 - 2^-70 -- the last
    # beside an odd c: the float64 sum is then the tie itself and rounding it again would go up to even, the exact sum goes down
    a2 = np.array([2.0 ** -12 + 2.0 ** -35, 2.0 ** -12, 1 + 2.0 ** -23], dtype=np.float32)
    b2 = np.array([2.0 ** -12 + 2.0 ** -35, 2.0 ** -12, 2.0 ** -24 * (1 - 2.0 ** -23)], dtype=np.float32)
    c2 = np.array([1, 1, 1 + 2.0 ** -23], dtype=np.float32)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got = pref.fmaf32(a, b, c)
    assert got.dtype == np.float32
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        err = abs(exact - Fraction(g))
        assert err <= abs(exact - Fraction(float(lo))) and err <= abs(exact - Fraction(float(hi))), (x, y, z, g)
    up = np.nextafter(np.float32(1), np.float32(2))
    assert got[-3] == up and got[-2] == 1.0 and got[-1] == up  # above the tie: up; the tie: to even; below the tie: down


def _update_loop(P, bank, labels, momentum, first):
    """the published script's shape: a loop over every sample accumulating class sums, then the rule class by class"""
    n = len(P)
    sums = [[0.0] * 512 for _ in range(n)]
    cnt = [0] * n
    for i in range(len(bank)):
        c = int(labels[i])
        if 0 <= c < n:
            cnt[c] += 1
            row = bank[i]
            s = sums[c]
            for k in range(512):
                s[k] += float(row[k])
    out = [list(map(float, P[c])) for c in range(n)]
    for c in range(n):
        if cnt[c]:
            for k in range(512):
                mean = sums[c][k] / cnt[c]
                out[c][k] = mean if first else (1.0 - momentum) * out[c][k] + momentum * mean
    return np.array(out), cnt


def test_update_rule_against_a_plain_loop():
    r = np.random.default_rng(3)
    n, N = 5, 40
    bank = np.abs(r.standard_normal((N, 512))).astype(np.float32)
    labels = r.integers(0, 4, N)  # class 4 stays empty
    labels[7], labels[9] = -1, 5  # two rows of no class
    P0 = np.zeros((n, 512), dtype=np.float32)
    P1, cnt, empty, bad = pref.update(P0, bank, labels, 0.2, True)
    want, wcnt = _update_loop(P0, bank, labels, 0.2, True)
    np.testing.assert_array_equal(P1, want)
    assert cnt.tolist() == wcnt and empty == 1 and bad == 2 and not P1[4].any()
    P1 = P1.astype(np.float32)
    bank2 = np.abs(r.standard_normal((N, 512))).astype(np.float32)
    P2, cnt2, empty2, _ = pref.update(P1, bank2, labels, 0.2, False)
    want2, _ = _update_loop(P1, bank2, labels, 0.2, False)
    np.testing.assert_array_equal(P2, want2)
    assert empty2 == 1 and not P2[4].any() and not np.array_equal(P2[:4], P1[:4])


def test_prototypes_argument_checks():
    from gdl.prototypes import Prototypes, prototype_logits

    import gdl

    assert gdl.Prototypes is Prototypes and gdl.prototype_logits is prototype_logits
    for n in (0, 513, -1, 6.0, True, None):
        with pytest.raises(L.GdlError, match="n_classes"):
            Prototypes(n, "cuda")
    for m in (-0.1, 1.5, float("nan")):
        with pytest.raises(L.GdlError, match="momentum"):
            Prototypes(6, "cuda", momentum=m)
    with pytest.raises(L.GdlError, match="no CPU path"):
        Prototypes(6, "cpu")
    with pytest.raises(L.GdlError, match="float32"):
        prototype_logits(torch.zeros(2, 256), torch.zeros(6, 512))
    with pytest.raises(L.GdlError, match="no CPU path"):
        prototype_logits(torch.zeros(2, 512), torch.zeros(6, 512))


def test_trainer_refusals_before_the_model():
    """What needs no look at the model is refused before the model is touched (there is none here): a wrong type, mode="dgl",
    a modulation beside the prototypes, a process group.  MODULATIONS is left as it was: prototypes= is a keyword of its own."""
    from gdl.prototypes import Prototypes
    from gdl.trainer import MODULATIONS, DGLTrainer

    assert MODULATIONS == ("Normal", "OGM", "OGM_GE")
    protos = Prototypes.__new__(Prototypes)  # (no device here: the checks in question look at the type alone)
    protos.n_classes = 6
    with pytest.raises(L.GdlError, match="gdl.Prototypes"):
        DGLTrainer(None, lr=1e-3, mode="joint", prototypes=torch.zeros(6, 512))
    with pytest.raises(L.GdlError, match="joint"):
        DGLTrainer(None, lr=1e-3, mode="dgl", prototypes=protos)
    with pytest.raises(L.GdlError, match="joint"):
        DGLTrainer(None, lr=1e-3, prototypes=protos)  # (the default mode is the DGL step)
    for mod in ("OGM", "OGM_GE"):
        with pytest.raises(L.GdlError, match="modulation"):
            DGLTrainer(None, lr=1e-3, mode="joint", modulation=mod, prototypes=protos)
    with pytest.raises(L.GdlError, match="process group"):
        DGLTrainer(None, lr=1e-3, mode="joint", prototypes=protos, process_group=object())
    DGLTrainer._check_prototypes(None, "dgl", "OGM", object())  # without prototypes nothing is checked


def test_abi_refusals_need_no_gpu():
    """n > 512, a width other than 512 and B < 1 are refused by the C ABI with GDL_ERR_ARG and a message before any launch."""
    lib = L.load()
    one = 0x1000  # (never dereferenced: the arguments are refused first)
    assert lib.gdl_proto_ce(one, one, one, one, one, None, 2, 513, 512, None) == 1 and b"n_classes" in lib.gdl_last_error()
    assert lib.gdl_proto_ce(one, one, one, one, one, None, 2, 6, 256, None) == 1 and b"width" in lib.gdl_last_error()
    assert lib.gdl_proto_ce(one, one, one, one, one, None, 0, 6, 512, None) == 1
    assert lib.gdl_proto_ce(one, None, one, one, one, None, 2, 6, 512, None) == 1
    assert lib.gdl_proto_apply(one, one, one, one, one, one, 1.0, one, 0, 512, None) == 1
    assert lib.gdl_proto_apply(one, one, one, one, one, one, 1.0, one, 4, 768, None) == 1 and b"width" in lib.gdl_last_error()
    assert lib.gdl_proto_apply(one, one, one + 4, one, one, one, 1.0, one, 4, 512, None) == 1 and b"aligned" in lib.gdl_last_error()
    assert lib.gdl_proto_update(one, one, 10, one, 513, 512, 0.2, 1, one, one, None) == 1
    assert lib.gdl_proto_update(one, one, 10, one, 6, 256, 0.2, 1, one, one, None) == 1
    assert lib.gdl_proto_update(one, one, 0, one, 6, 512, 0.2, 1, one, one, None) == 1
    assert lib.gdl_proto_update(one, one, 10, one, 6, 512, 1.2, 1, one, one, None) == 1 and b"momentum" in lib.gdl_last_error()
