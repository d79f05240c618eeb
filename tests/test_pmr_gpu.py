"""GPU tests of prototypical modal rebalance (csrc/proto.hip, gdl.prototypes, DGLTrainer(prototypes=...)): the three launches
against the float64 restatement of tests/pmr_ref.py (pinned on the CPU by tests/test_pmr_cpu.py) with ITS derived bounds, the
float32 mirrors where the bits are the contract, the trainer against the reference-built step goldens
(tests/golden/make_golden_pmr.py) and against a Normal joint trainer from the same seed, the switches, checkpoints and refusals."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pmr_ref as pref  # noqa: E402
from gdl import _lib as L  # noqa: E402
from gpu_util import DEV, dev  # noqa: E402

from oracle import fixtures as fx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _same_f32(got, want):
    """float32 arrays equal bit for bit where finite, NaN where NaN (a NaN's payload is not part of any contract)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)))


# ------------------------------------------------------------------ gdl_proto_ce
def _features(seed, B, n, scale):
    """0.5 |N(0, 1)| features and prototypes -- what post-ReLU pooled features look like: d ~ 10 (scale 8: d ~ 87)"""
    r = np.random.default_rng([97, seed])
    f = (0.5 * scale * np.abs(r.standard_normal((B, 512)))).astype(np.float32)
    P = (0.5 * scale * np.abs(r.standard_normal((n, 512)))).astype(np.float32)
    return f, P, r.integers(0, n, B)


def _proto_ce(f, P, labels, sim=True):
    B, n = f.shape[0], P.shape[0]
    u = torch.full((B, 512), float("nan"), device=DEV)
    terms = torch.full((2, B), float("nan"), device=DEV)
    s = torch.full((B, n), float("nan"), device=DEV) if sim else None
    L.call("gdl_proto_ce", L.ptr(f), L.ptr(P), L.ptr(labels), L.ptr(u), L.ptr(terms), L.ptr(s), B, n, 512, L.cur_stream())
    return u, terms, s


CE_CASES = [  # B, n, scale, special
    (1, 1, 1.0, None),            # one class: p = 1, u = 0
    (3, 6, 1.0, "label -1"),      # fewer classes than waves
    (5, 17, 1.0, "on prototype"),  # the odd tail of the two-at-a-time class loop
    (4, 33, 1.0, "label n"),      # the wrap past 32 classes
    (2, 512, 1.0, None),          # the LDS cap
    (64, 309, 1.0, None),         # the workload's own shape
    (5, 17, 8.0, None),           # d ~ 87: the bound grows with d_max
]


@pytest.mark.parametrize("B,n,scale,special", CE_CASES)
def test_proto_ce(B, n, scale, special):
    """gdl_proto_ce against the float64 restatement, within the bounds tests/pmr_ref.py derives from the kernel's sum orders
    (u = 2^-24, T = 16 u per expf / logf / division as in tests/head_ref.py):
      |dsim|            <= C_D u d,  C_D = (3 + 8 + 6) / 2 + 1 = 9.5 -- three roundings per squared difference, the 8 fmaf of a
                           lane's chain, the 6 adds of the butterfly, halved by the square root, plus its rounding
      |dp| / p          <= 2 C_D u d_max + 3 u d_max + (n + 2 T + T ln n + ln n) u        (eps_p)
      |d loss term|     <= 2 C_D u d_max + 2 u d_max + (n + T + T ln n) u + u |term|
      |dq_j|            <= (p_j eps_p + (1 + 2 T + C_D) u |p_j - onehot_j|) / (B d_j)
      |du_k|            <= sum_j |dq_j| |P_jk - f_k| + (n + 1) u sum_j |q_j| |P_jk - f_k|
    evaluated per element from the float64 values.  Each case runs twice on the same buffers: identical bits.  Specials: a
    label of n, a label of -1 (no one-hot term, score term 0, NaN loss term), a feature row ON a prototype (q = 0 there, u
    finite).  The largest observed error-to-bound ratios are printed (docs/parity_log.md records them)."""
    f, P, labels = _features(1000 * B + n + int(scale), B, n, scale)
    if special == "label n":
        labels[0] = n
    if special == "label -1":
        labels[2] = -1
    if special == "on prototype":
        f[1] = P[4]
    fd, Pd, ld = dev(f), dev(P), torch.from_numpy(labels).to(DEV)
    u, terms, sim = _proto_ce(fd, Pd, ld)
    u2, terms2, sim2 = _proto_ce(fd, Pd, ld)
    u3, terms3, _ = _proto_ce(fd, Pd, ld, sim=False)  # (the sim store is optional and changes nothing else)
    torch.cuda.synchronize()
    assert _same_bits(u, u2) and _same_bits(sim, sim2) and _same_f32(terms.cpu().numpy(), terms2.cpu().numpy())
    assert _same_bits(u, u3) and _same_f32(terms.cpu().numpy(), terms3.cpu().numpy())
    r = pref.proto_ce(f, P, labels)
    b = pref.proto_ce_bounds(r, B)
    got = dict(sim=sim.cpu().numpy().astype(np.float64), u=u.cpu().numpy().astype(np.float64),
               term_p=terms[0].cpu().numpy().astype(np.float64), term_l=terms[1].cpu().numpy().astype(np.float64))
    ok = ~np.isnan(r["term_l"])
    assert np.array_equal(np.isnan(got["term_l"]), ~ok)           # a label outside [0, n): NaN loss term ...
    assert (got["term_p"][~ok] == 0).all()                        # ... and a score term of 0
    assert np.isfinite(got["u"]).all() and np.isfinite(got["sim"]).all()
    want = dict(sim=r["sim"], u=r["u"], term_p=r["term_p"], term_l=np.where(ok, r["term_l"], 0.0))
    got["term_l"] = np.where(ok, got["term_l"], 0.0)
    ratios = {k: float((np.abs(got[k] - want[k]) / b[k]).max()) for k in ("sim", "term_p", "term_l", "u")}
    print(f"proto_ce B={B} n={n} scale={scale} d_max={r['d'].max():.1f} error/bound:", {k: round(v, 4) for k, v in ratios.items()},
          "max |dsim| / (u d):", float((np.abs(got["sim"] - want["sim"]) / (pref.U * np.maximum(r["d"], 1e-30))).max()))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    if special == "on prototype":
        assert got["sim"][1, 4] == 0.0 and r["q"][1, 4] == 0.0
    assert (~ok).sum() == (1 if special in ("label n", "label -1") else 0)
    if n == 1:
        assert (got["u"] == 0).all() and (got["term_p"] == 1).all()


def test_proto_ce_refusals():
    f, P, labels = _features(1, 2, 6, 1.0)
    fd, Pd, ld = dev(f), dev(P), torch.from_numpy(labels).to(DEV)
    u, terms = torch.zeros((2, 512), device=DEV), torch.zeros((2, 2), device=DEV)
    lib = L.load()
    st = L.cur_stream()
    big = torch.zeros((513, 512), device=DEV)
    assert lib.gdl_proto_ce(L.ptr(fd), L.ptr(big), L.ptr(ld), L.ptr(u), L.ptr(terms), None, 2, 513, 512, st) == 1  # GDL_ERR_ARG
    assert lib.gdl_proto_ce(L.ptr(fd), L.ptr(Pd), L.ptr(ld), L.ptr(u), L.ptr(terms), None, 2, 6, 256, st) == 1
    assert lib.gdl_proto_ce(L.ptr(fd), L.ptr(Pd), L.ptr(ld), L.ptr(u), L.ptr(terms), None, 0, 6, 512, st) == 1
    torch.cuda.synchronize()
    assert not u.any() and not terms.any()  # nothing was launched


def test_prototype_logits():
    import gdl

    f, P, labels = _features(2, 5, 17, 1.0)
    fd, Pd = dev(f), dev(P)
    sim = gdl.prototype_logits(fd, Pd)
    _, _, want = _proto_ce(fd, Pd, torch.from_numpy(labels).to(DEV))
    assert _same_bits(sim, want)
    with pytest.raises(L.GdlError):
        gdl.prototype_logits(fd[:, :256].contiguous(), Pd)
    with pytest.raises(L.GdlError):
        gdl.prototype_logits(fd, torch.zeros((513, 512), device=DEV))


# ------------------------------------------------------------------ gdl_proto_apply
ALPHA = 0.7


def _terms(seed, B, kind):
    """terms_a, terms_v [2, B] float32: label probabilities in (0, 1) and positive loss terms"""
    r = np.random.default_rng([53, seed, B])
    ta = np.stack([r.random(B) * 0.9 + 0.05, r.random(B) * 3 + 0.1]).astype(np.float32)
    tv = np.stack([r.random(B) * 0.9 + 0.05, r.random(B) * 3 + 0.1]).astype(np.float32)
    if kind == "audio":     # audio ahead: the visual probabilities are the audio ones in another order, halved (rho = 2)
        tv[0] = r.permutation(ta[0]) * np.float32(0.5)
    elif kind == "visual":  # rho = 1 / 2
        ta[0] = r.permutation(tv[0]) * np.float32(0.5)
    elif kind == "one":     # rho exactly 1
        tv[0] = ta[0]
    elif kind == "zero":    # score_v = 0: rho = inf, audio "ahead"
        tv[0] = 0
    elif kind == "nan":     # a NaN term (a label outside [0, n) gives a NaN LOSS term; a NaN score needs NaN features)
        ta[0, B // 2] = np.nan
    return ta, tv


APPLY_CASES = [(B, kind) for B in (1, 3, 64, 300) for kind in ("audio", "visual")] + [(64, "one"), (3, "zero"), (300, "nan")]


@pytest.mark.parametrize("B,kind", APPLY_CASES)
def test_proto_apply(B, kind):
    """stats[8] bit for bit against the float32 mirror of the fold (pref.apply_stats: ticket_fold256's order, the stride past
    256 at B = 300); the side whose coefficient is 0 keeps its df bits; the other side is fmaf(coefficient, u, df) bit for bit
    (pref.fmaf32).  The audio / visual cases have |rho - 1| >= 1e-3 in the float64 restatement (asserted); rho == 1, score_v = 0
    and a NaN term each get a case: both coefficients 0, lam = alpha (rho = +inf), both 0."""
    ta, tv = _terms(7, B, kind)
    r = np.random.default_rng([59, B])
    ua, uv, dfa, dfv = (r.standard_normal((B, 512)).astype(np.float32) for _ in range(4))
    rho64, beta64, lam64 = pref.coefficients(ta[0].astype(np.float64).sum(), tv[0].astype(np.float64).sum(), ALPHA)
    if kind in ("audio", "visual"):
        assert abs(rho64 - 1) >= 1e-3 and (rho64 > 1) == (kind == "audio")
    want = pref.apply_stats(ta, tv, ALPHA)
    beta, lam = want[3], want[4]
    if kind in ("audio", "visual"):
        assert (beta, lam) == ((0, np.float32(ALPHA)) if kind == "audio" else (np.float32(ALPHA), 0)) and beta == np.float32(beta64)
    elif kind == "zero":
        assert np.isinf(want[2]) and beta == 0 and lam == np.float32(ALPHA)
    else:
        assert beta == 0 and lam == 0 and (want[2] == 1 if kind == "one" else np.isnan(want[2]))
    tad, tvd, uad, uvd, dad, dvd = (dev(x) for x in (ta, tv, ua, uv, dfa, dfv))
    stats = torch.full((8,), float("nan"), device=DEV)
    outs = []
    for _ in range(2):  # twice from the same inputs: identical bytes
        da, dv = dad.clone(), dvd.clone()
        L.call("gdl_proto_apply", L.ptr(tad), L.ptr(tvd), L.ptr(uad), L.ptr(uvd), L.ptr(da), L.ptr(dv), ALPHA, L.ptr(stats), B, 512,
               L.cur_stream())
        outs.append((da, dv, stats.clone()))
    torch.cuda.synchronize()
    (da, dv, s), (da2, dv2, s2) = outs
    assert _same_bits(da, da2) and _same_bits(dv, dv2) and _same_f32(s.cpu().numpy(), s2.cpu().numpy())
    print("proto_apply", B, kind, "stats", s.cpu().numpy(), "mirror", want)
    assert _same_f32(s.cpu().numpy(), want)
    for got, df0, u, coef in ((da, dfa, ua, beta), (dv, dfv, uv, lam)):
        if coef == 0:
            assert _same_f32(got.cpu().numpy(), df0)
        else:
            assert _same_f32(got.cpu().numpy(), pref.fmaf32(coef, u, df0))
            assert not _same_f32(got.cpu().numpy(), df0)


# ------------------------------------------------------------------ gdl_proto_update
def _bank(seed, N, n, skew):
    r = np.random.default_rng([61, seed, N])
    bank = np.abs(r.standard_normal((N, 512))).astype(np.float32) * np.float32(0.5)
    labels = r.integers(0, n, N)
    if skew:  # a few rows of no class
        labels[5], labels[6] = -1, n
    return bank, labels


def _ulp_close(got, want64):
    w = want64.astype(np.float32)
    return bool((np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(w)).astype(np.float64)).all())


@pytest.mark.parametrize("N,n", [(1, 6), (7, 6), (1000, 6), (700, 309)])
def test_proto_update(N, n):
    """The first call (P_c = mean_c) and a momentum call on another bank, against pref.update: every prototype within one
    float32 unit in the last place of the float64 value, counts, the number of empty classes and of rows of no class exact, an
    empty class keeps its bits (the buffer starts from a pattern, not from zero, to show it), two runs give identical bytes.
    N = 700 with n = 309 leaves classes empty for certain; N = 1000 spans two chunks of the kernel's 512-row walk and has two rows
    whose label is outside [0, n)."""
    banks = [_bank(1, N, n, N == 1000), _bank(2, N, n, False)]
    P0 = np.random.default_rng(67).standard_normal((n, 512)).astype(np.float32)
    runs = []
    for _ in range(2):
        P = dev(P0)
        count = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        info = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        snaps = []
        for k, (bank, labels) in enumerate(banks):
            bd, ld = dev(bank), torch.from_numpy(labels).to(DEV)  # (named: they must outlive the launch)
            L.call("gdl_proto_update", L.ptr(bd), L.ptr(ld), N, L.ptr(P), n, 512, 0.2, int(k == 0), L.ptr(count), L.ptr(info),
                   L.cur_stream())
            torch.cuda.synchronize()
            snaps.append((P.cpu().numpy().copy(), count.cpu().numpy().copy(), info.cpu().numpy().copy()))
        runs.append(snaps)
    Pw = P0
    for k, (bank, labels) in enumerate(banks):
        got, cnt, info = runs[0][k]
        P64, wcnt, empty, bad = pref.update(Pw, bank, labels, 0.2, k == 0)
        assert np.array_equal(cnt, wcnt) and info.tolist() == [empty, bad]
        assert _ulp_close(got, P64), float(np.abs(got - P64).max())
        keep = wcnt == 0
        assert np.array_equal(got[keep].view(np.int32), Pw[keep].view(np.int32))
        assert np.array_equal(got.view(np.int32), runs[1][k][0].view(np.int32)) and np.array_equal(cnt, runs[1][k][1])
        if n == 309:
            assert empty > 0
        if N == 1000 and k == 0:
            assert bad == 2
        Pw = got  # the momentum call starts from the device's float32 prototypes
    assert not np.array_equal(runs[0][0][0], runs[0][1][0])


def test_prototypes_class():
    """gdl.Prototypes over two FeatureBanks: the first update sets, the second applies the momentum; state_dict round trip;
    check() reports rows of no class; a bank of another kind is refused."""
    import gdl

    n, N = 6, 40
    protos = gdl.Prototypes(n, DEV)
    assert protos.audio.shape == (n, 512) and not protos.protos.any() and protos.count.shape == (2, n) and protos.updates == 0
    Pw = np.zeros((2, n, 512), dtype=np.float32)
    for k in range(2):
        banks = [_bank(10 + 2 * k + m, N, n - 1, False) for m in range(2)]  # class 5 has no row
        fb = [gdl.FeatureBank(dev(b), torch.from_numpy(lab).to(DEV), mod) for (b, lab), mod in zip(banks, ("audio", "visual"))]
        protos.update(*fb)
        for m in range(2):
            P64, cnt, empty, bad = pref.update(Pw[m], banks[m][0], banks[m][1], 0.2, k == 0)
            got = protos.protos[m].cpu().numpy()
            assert _ulp_close(got, P64) and np.array_equal(protos.count[m].cpu().numpy(), cnt)
            assert protos.info[m].tolist() == [1, 0] and int(protos.empty[m]) == 1
            Pw[m] = got
        assert protos.updates == k + 1
    assert protos.check() == {"empty": [1, 1]}
    other = gdl.Prototypes(n, DEV, momentum=0.5)
    other.load_state_dict(protos.state_dict())
    assert _same_bits(other.protos, protos.protos) and other.updates == 2 and other.momentum == 0.2
    with pytest.raises(L.GdlError, match="classes"):
        gdl.Prototypes(7, DEV).load_state_dict(protos.state_dict())
    with pytest.raises(L.GdlError, match="FeatureBank"):
        protos.update(fb[0], fb[1].features)
    with pytest.raises(L.GdlError, match="visual"):
        protos.update(fb[1], fb[1])
    bad_lab = banks[0][1].copy()
    bad_lab[3] = n
    protos.update(gdl.FeatureBank(dev(banks[0][0]), torch.from_numpy(bad_lab).to(DEV)), fb[1])
    with pytest.raises(L.GdlError, match="outside"):
        protos.check()


# ------------------------------------------------------------------ the runner
_STATE = {}
_TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3)
_FIXSTATE = {"concat": "concat", "sum": "sum_dgl", "gated": "gated_dgl", "film": "film_dgl"}


def _state(n_classes, fusion):
    if (n_classes, fusion) not in _STATE:
        P, Bf = fx.model_state(n_classes, _FIXSTATE[fusion])
        _STATE[(n_classes, fusion)] = {k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()}
    return _STATE[(n_classes, fusion)]


def _make_model(cfg, dtype="f32"):
    from models.basic_model import AVClassifier

    args = argparse.Namespace(fusion_method=cfg["fusion"], dataset=cfg["dataset"], modality="full", batch_size=cfg["batch"])
    model = AVClassifier(args)
    model.load_state_dict(_state(cfg["n_classes"], cfg["fusion"]), strict=True)
    model = model.to(DEV)
    model.audio_net.gdl_dtype = dtype
    model.visual_net.gdl_dtype = dtype
    return model.train()


def _batch(cfg, st):
    spec, image, label = fx.make_batch(cfg["seed"] + st, cfg["batch"], cfg["spec_hw"], cfg["frames"], cfg["image_hw"],
                                       cfg["n_classes"])
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _trainer(cfg, dtype="f32", **kw):
    from gdl.trainer import DGLTrainer

    model = _make_model(cfg, dtype)
    return model, DGLTrainer(model, lr=cfg["lr"], mode="joint", **kw)


def _protos(P, n=6):
    import gdl

    p = gdl.Prototypes(n, DEV)
    p.protos.copy_(torch.as_tensor(P))
    p.updates = 1
    return p


def _pick_prototypes(fa, fv, label, n, audio_leads, seed0):
    """0.5 |N(0, 1)| prototypes [2, n, 512] from the first seed at which the restatement has the wanted side ahead by 5 %"""
    for k in range(1000):
        r = np.random.default_rng([71, seed0, k])
        P = (0.5 * np.abs(r.standard_normal((2, n, 512)))).astype(np.float32)
        rho = pref.proto_ce(fa, P[0], label)["score"] / pref.proto_ce(fv, P[1], label)["score"]
        if (rho > 1.05) if audio_leads else (rho < 0.95):
            return P
    raise AssertionError("no prototype seed gives the wanted lead")


@pytest.mark.parametrize("fusion,audio_leads", [("concat", True), ("sum", False), ("gated", True), ("film", False)])
def test_step_against_normal_trainer(fusion, audio_leads):
    """One f32 step of DGLTrainer(mode="joint", prototypes=...) beside a Normal joint trainer from the same state and batch, for
    each of the four heads (the leading side alternates).  The logits, loss_f and the head's parameter gradients are the Normal
    step's bits; read()["pmr"] matches the restatement evaluated on the trainer's own fa / fv (scores and losses within the
    summed per-sample bounds of tests/pmr_ref.py plus (B + 9) u for the fold and the division; rho within the two scores'
    relative bounds plus u; beta / lam exact); the helped side's feature gradient is fmaf(alpha, u, Normal's) bit for bit with u
    within its bound; the encoder on the side with coefficient 0 has every weight gradient bit-identical to the Normal
    trainer's, the other encoder's gradients are not.  Both trainers run with max_norm = 1e6: the update writes the CLIPPED
    gradient back to the arena `tr.grad(name)` reads, and the clip coefficient comes from the total norm, which the prototype
    term changes -- with the clip idle (coefficient exactly 1) the arena holds the gradients as the backward left them.
    (Fails without the feature: `prototypes` is no keyword there.)"""
    cfg = dict(_TINY, fusion=fusion)
    spec, image, label = _batch(cfg, 0)
    alpha = 1.5
    mn, trn = _trainer(cfg, max_norm=1e6)
    trn.step(spec, image, label)
    rn = trn.read()
    assert rn["clip_coef"] == 1.0
    fa, fv, lab = trn.fa.cpu().numpy(), trn.fv.cpu().numpy(), label.cpu().numpy()
    P = _pick_prototypes(fa, fv, lab, 6, audio_leads, 3)
    mp, tr = _trainer(cfg, prototypes=_protos(P), alpha=alpha, max_norm=1e6)
    tr.step(spec, image, label)
    r = tr.read()
    assert r["clip_coef"] == 1.0 and "pmr" not in rn and _same_bits(tr.fa, trn.fa) and _same_bits(tr.fv, trn.fv)
    np.testing.assert_array_equal(r["out"], rn["out"])
    assert r["loss_f"] == rn["loss_f"]
    B, U = 4, pref.U
    ra, rv = pref.proto_ce(fa, P[0], lab), pref.proto_ce(fv, P[1], lab)
    ba, bv = pref.proto_ce_bounds(ra, B), pref.proto_ce_bounds(rv, B)
    o = r["pmr"]
    print(fusion, "pmr", o, "float64", ra["score"], rv["score"], ra["lossp"], rv["lossp"])
    rel = {}
    for m, rr, bb in (("a", ra, ba), ("v", rv, bv)):
        tol_s = bb["term_p"].sum() + (B + 9) * U * rr["score"]
        assert abs(o["score_" + m] - rr["score"]) <= tol_s, (m, o, rr["score"])
        assert abs(o["lossp_" + m] - rr["lossp"]) <= bb["term_l"].sum() / B + (B + 9) * U * abs(rr["lossp"])
        rel[m] = tol_s / rr["score"]
    rho, beta, lam = pref.coefficients(ra["score"], rv["score"], alpha)
    assert abs(o["rho"] - rho) <= (rel["a"] + rel["v"] + 2 * U) * rho
    assert (o["beta"], o["lam"]) == (beta, lam) == ((0.0, alpha) if audio_leads else (alpha, 0.0))
    # the helped side's feature gradient: Normal's, plus alpha u in one fused multiply-add
    m = 1 if audio_leads else 0
    df, dfn, rr, bb = ((tr.dfa, trn.dfa, ra, ba), (tr.dfv, trn.dfv, rv, bv))[m]
    ug = tr.pmr_u[m].cpu().numpy()
    assert (np.abs(ug - rr["u"]) <= bb["u"]).all() and np.abs(ug).max() > 0
    assert _same_f32(df.cpu().numpy(), pref.fmaf32(np.float32(alpha), ug, dfn.cpu().numpy()))
    other = (tr.dfv, trn.dfv) if m == 0 else (tr.dfa, trn.dfa)
    assert _same_bits(*other)
    kept, helped = ("audio_net.", "visual_net.") if audio_leads else ("visual_net.", "audio_net.")
    differ = total = 0
    for name in trn.names:
        same = _same_bits(tr.grad(name), trn.grad(name))
        if name.startswith(helped):
            total += 1
            differ += not same
        else:  # the encoder with coefficient 0, and the head: no gradient from the prototype terms
            assert same, name
    assert total == 60 and differ >= 50, (differ, total)
    assert not _same_bits(tr.params, trn.params)
    tr.close()
    trn.close()


GOLDENS = ["pmr_concat_tiny_b4", "pmr_sum_tiny_b4"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", GOLDENS)
def test_pmr_step_golden(name, dtype):
    """DGLTrainer(mode="joint", prototypes=...) against the step built from the reference's encoders and heads under torch
    autograd with the prototype term in torch (tests/golden/make_golden_pmr.py; two steps, each side leads once), with the
    constants of tests/test_modulation_gpu.py::test_ogm_step_golden: f32 -- per step the logits, loss, total norm, gradient sums
    and per-tensor norms, the final parameter sums, buffers and eval logits; the scores within 1e-3 absolute at step 0 (|dp| <=
    max |dsim| / 2 per sample, times B = 4, at that test's 5e-4 logit bound; 2e-2 at step 1 with its 1e-2), the prototype
    losses within the loss tolerance, rho within (1 + rho) times the score tolerance / min(score), beta and lam exact.  bf16:
    everything finite (the 5 % lead of the fixture is inside bf16's feature error, so the side is not asserted)."""
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    assert cfg["method"] == "PMR" and cfg["steps"] == 2
    protos = _protos(g["s0.prototypes"])
    model, tr = _trainer(cfg, dtype, alpha=cfg["alpha"], prototypes=protos, modulation_starts=cfg["modulation_starts"],
                         modulation_ends=cfg["modulation_ends"])
    f32 = dtype == "f32"
    leads = []
    for st in range(cfg["steps"]):
        pre = f"s{st}."
        protos.protos.copy_(torch.from_numpy(g[pre + "prototypes"]))
        spec, image, label = _batch(cfg, st)
        tr.step(spec, image, label)
        r = tr.read()
        later = st > 0
        o = r["pmr"]
        want = {k: float(g[pre + k]) for k in ("score_a", "score_v", "rho", "beta", "lam", "lossp_a", "lossp_v")}
        print(name, dtype, st, o, "golden", want)
        leads.append(want["rho"] > 1)
        assert all(np.isfinite(v) for v in o.values())
        if not f32:
            assert np.isfinite(r["out"]).all() and np.isfinite(r["total_norm"]) and np.isfinite(r["loss_f"])
            continue
        lt = 1e-2 if later else 5e-4
        stol = 2 * lt
        assert abs(o["score_a"] - want["score_a"]) < stol and abs(o["score_v"] - want["score_v"]) < stol
        assert abs(o["rho"] - want["rho"]) <= (1 + want["rho"]) * stol / min(want["score_a"], want["score_v"])
        assert (o["beta"], o["lam"]) == (want["beta"], want["lam"])
        np.testing.assert_allclose([o["lossp_a"], o["lossp_v"]], [want["lossp_a"], want["lossp_v"]], rtol=lt, atol=lt)
        print(name, dtype, st, "logits", float(np.abs(r["out"] - g[pre + "out"]).max()), "loss", r["loss_f"], float(g[pre + "loss_f"]),
              "total_norm", r["total_norm"], float(g[pre + "total_norm"]))
        np.testing.assert_allclose(r["out"], g[pre + "out"], rtol=lt, atol=lt)
        np.testing.assert_allclose(r["loss_f"], g[pre + "loss_f"], rtol=lt, atol=lt)
        nt = 2e-2 if later else 3e-3
        tn = float(g[pre + "total_norm"])
        np.testing.assert_allclose(r["total_norm"], tn, rtol=nt)
        np.testing.assert_allclose(r["audio_grad_sum"], g[pre + "audio_grad_sum"], rtol=2 * nt)
        np.testing.assert_allclose(r["visual_grad_sum"], g[pre + "visual_grad_sum"], rtol=2 * nt)
        gt = 6e-2 if later else 1e-2
        clip = min(1.0, 40.0 / (tn + 1e-6))
        assert clip < 1.0  # the clip is active in these fixtures
        for i, n in enumerate(str(x) for x in g[pre + "grad_names"]):
            w = float(g[pre + "grad_norm"][i]) * clip
            assert abs(r["grad_norm"][n] - w) <= gt * w + 1e-5 * clip * tn, (n, r["grad_norm"][n], w)
    assert leads == [True, False]  # each fixture exercises both branches
    if not f32:
        assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
        tr.close()
        return
    last = f"s{cfg['steps'] - 1}."
    names = [str(n) for n in g[last + "grad_names"]]
    sd = model.state_dict()
    for i, n in enumerate(names):
        np.testing.assert_allclose(sd[n].double().abs().sum().item(), g[last + "param_sums"][i][1], rtol=1e-3, err_msg=n)
    for k in [k[len(last + "buf."):] for k in g.files if k.startswith(last + "buf.")]:
        np.testing.assert_allclose(sd[k].cpu().numpy().astype(np.float64), g[last + "buf." + k], rtol=2e-3, atol=1e-3, err_msg=k)
    model.eval()
    spec, image, label = _batch(cfg, 1000)
    with torch.no_grad():
        ev = model(spec.unsqueeze(1), image)[2]
    np.testing.assert_allclose(ev.cpu().numpy(), g["eval.out"], rtol=1e-2, atol=1e-2)
    tr.close()


@pytest.mark.parametrize("how", ["none", "window"])
def test_switched_off_is_bit_identical(how):
    """prototypes=None, or an epoch outside the window, is the step of a trainer built without the new argument, bit for bit --
    parameters, gradients, momentum, statistics, over two steps -- and nothing of PMR's is allocated."""
    from gdl.trainer import DGLTrainer

    cfg = dict(_TINY, fusion="concat")
    m0 = _make_model(cfg)
    t0 = DGLTrainer(m0, lr=cfg["lr"], mode="joint")
    P = (0.5 * np.abs(np.random.default_rng(5).standard_normal((2, 6, 512)))).astype(np.float32)
    kw = dict(prototypes=None) if how == "none" else dict(prototypes=_protos(P), alpha=1.0, modulation_starts=2, modulation_ends=3)
    m1, t1 = _trainer(cfg, **kw)
    for st in range(2):  # (window: the default epoch 0 is in front of it, epoch 4 behind)
        b = _batch(cfg, st)
        t0.step(*b)
        t1.step(*b)
        if how == "window" and st == 0:
            t1.epoch = 4
        r0, r1 = t0.read(), t1.read()
        assert "pmr" not in r1
        np.testing.assert_array_equal(r0["out"], r1["out"])
        assert _same_bits(t0.stats, t1.stats) and _same_bits(t0.grads, t1.grads)
        assert _same_bits(t0.params, t1.params) and _same_bits(t0.momentum, t1.momentum)
    assert t1._pmr_B is None and not hasattr(t1, "pmr_u")
    assert ("prototypes" in t1.state_dict()) == (how == "window")
    t0.close()
    t1.close()


def test_window_switches_the_term_on():
    cfg = dict(_TINY, fusion="sum")
    P = (0.5 * np.abs(np.random.default_rng(6).standard_normal((2, 6, 512)))).astype(np.float32)
    _, t = _trainer(cfg, prototypes=_protos(P), alpha=1.0, modulation_starts=1, modulation_ends=1)
    t.step(*_batch(cfg, 0))
    assert "pmr" not in t.read()
    t.epoch = 1
    t.step(*_batch(cfg, 1))
    o = t.read()["pmr"]
    assert set(o) == {"score_a", "score_v", "rho", "beta", "lam", "lossp_a", "lossp_v"} and o["beta"] + o["lam"] == 1.0
    t.epoch = 2
    t.step(*_batch(cfg, 0))
    assert "pmr" not in t.read()
    t.close()


def test_checkpoint_round_trip():
    """state_dict() carries the prototypes' state; a fresh trainer with fresh prototypes continues bit-identically; a
    checkpoint with prototypes is refused by a trainer without them, and the reverse."""
    from gdl.trainer import DGLTrainer

    import gdl

    cfg = dict(_TINY, fusion="concat")
    P = (0.5 * np.abs(np.random.default_rng(8).standard_normal((2, 6, 512)))).astype(np.float32)
    m0, t0 = _trainer(cfg, prototypes=_protos(P), alpha=1.0)
    t0.step(*_batch(cfg, 0))
    ck_model = {k: v.clone() for k, v in m0.state_dict().items()}
    ck = t0.state_dict()
    assert ck["steps"] == 1 and ck["prototypes"]["updates"] == 1 and "modulation" not in ck
    m1 = _make_model(cfg)
    m1.load_state_dict(ck_model)
    fresh = gdl.Prototypes(6, DEV)
    t1 = DGLTrainer(m1, lr=cfg["lr"], mode="joint", prototypes=fresh, alpha=1.0)
    t1.load_state_dict(ck)
    assert t1.steps == 1 and fresh.updates == 1 and _same_bits(fresh.protos, t0.prototypes.protos)
    b = _batch(cfg, 1)
    t0.step(*b)
    t1.step(*b)
    assert t0.read()["pmr"] == t1.read()["pmr"]
    assert _same_bits(t0.grads, t1.grads) and _same_bits(t0.params, t1.params) and _same_bits(t0.momentum, t1.momentum)
    m2, t2 = _trainer(cfg)
    with pytest.raises(L.GdlError, match="prototypes"):
        t2.load_state_dict(ck)
    with pytest.raises(L.GdlError, match="prototypes"):
        t1.load_state_dict(t2.state_dict())
    for t in (t0, t1, t2):
        t.close()


def test_refusals():
    """What the prototype term is not built for raises instead of being ignored: mode="dgl", a modulation beside it, the Swin
    composition, a process group, prototypes of another class count or on another device, something that is no gdl.Prototypes."""
    import gdl
    from gdl.trainer import DGLTrainer
    from models.basic_model import AVClassifier, AVClassifier_DGL, AVClassifier_DGL_Swin

    def ns(fusion):
        return argparse.Namespace(fusion_method=fusion, dataset="CREMAD", modality="full", batch_size=4)

    protos = gdl.Prototypes(6, DEV)
    joint = AVClassifier(ns("concat")).to(DEV)
    with pytest.raises(L.GdlError, match="joint"):
        DGLTrainer(AVClassifier_DGL(ns("concat")).to(DEV), lr=1e-3, mode="dgl", prototypes=protos)
    for mod in ("OGM", "OGM_GE"):
        with pytest.raises(L.GdlError, match="modulation"):
            DGLTrainer(joint, lr=1e-3, mode="joint", modulation=mod, prototypes=protos)
    with pytest.raises(L.GdlError, match="process group"):
        DGLTrainer(joint, lr=1e-3, mode="joint", prototypes=protos, process_group=object())
    with pytest.raises(L.GdlError, match="classes"):
        DGLTrainer(joint, lr=1e-3, mode="joint", prototypes=gdl.Prototypes(7, DEV))
    elsewhere = gdl.Prototypes(6, DEV)
    elsewhere.device = torch.device("cuda", 1)  # (what prototypes built on another card report; no second card is needed)
    with pytest.raises(L.GdlError, match="cuda:1"):
        DGLTrainer(joint, lr=1e-3, mode="joint", prototypes=elsewhere)
    with pytest.raises(L.GdlError, match="gdl.Prototypes"):
        DGLTrainer(joint, lr=1e-3, mode="joint", prototypes=protos.protos)
    sc = fx.SWIN_TINY2
    swin = AVClassifier_DGL_Swin(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality="full", pe=0),
                                 swin_kwargs=dict(img_size=sc["img"], patch_size=sc["patch"], embed_dim=sc["embed"],
                                                  depths=list(sc["depths"]), num_heads=list(sc["heads"]),
                                                  window_size=sc["window"], mlp_ratio=float(sc["mlp"]), drop_path_rate=0.)).to(DEV)
    with pytest.raises(L.GdlError, match="Swin"):
        DGLTrainer(swin, lr=1e-3, mode="joint", prototypes=protos)
    # accepted where it is built: every joint head
    for fusion in ("concat", "sum", "gated"):
        DGLTrainer(AVClassifier(ns(fusion)).to(DEV), lr=1e-3, mode="joint", prototypes=protos).close()
