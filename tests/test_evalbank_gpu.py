"""GPU tests of the evaluation report's score bank (csrc/evalbank.hip, gdl/evaluate.py) against the restatement of
tests/evalbank_ref.py: integer outputs exactly, stored probabilities inside the derived bound, average precision against the
exact rational value computed from the probabilities the kernel itself stored, scikit-learn's recorded values, run-to-run
identical bytes, untouched sentinels, and the three runners' `valid(batches, bank=...)` / `score(..., scores=...)`.

Measured on MI355X (docs/parity_log.md "score bank"): the worst stored probability lies at 0.65 of its bound (subnormal
values of the spread logits, against the bound's floor), 0.27 for the other kinds of scores."""
import argparse
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import evalbank_ref as er
from gdl import _lib as L
from gpu_util import DEV, dev
from oracle import fixtures as fx

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evalbank_small.npz")
GUARD, FILL = 4096, 0xA5
NS = (1, 63, 64, 65, 257, 1000)
CLASSES = (1, 2, 6, 65, 309, 512)
WORST = {"probs": 0.0}


def run_bank(logit_sets, labels, n, capacity=None, chunks=None):
    """A ScoreBank whose buffer sits between sentinels, everything but its counters pre-filled with the sentinel byte;
    appends in `chunks`, one report.  -> (bank, report, labels, probs, bytes of the bank)"""
    import gdl

    N, S = len(labels), len(logit_sets)
    capacity = N if capacity is None else capacity
    bank = gdl.ScoreBank(n, capacity, S, DEV)
    nbytes = bank.buf.numel()
    big = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    bank.buf = big[GUARD:GUARD + nbytes]
    bank.reset()
    ld = [dev(np.asarray(l, dtype=np.float32)) for l in logit_sets] + [None] * (3 - S)
    lab = torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(DEV)
    o = 0
    for B in chunks or [N]:
        bank.append(*(t[o:o + B] if t is not None else None for t in ld), lab[o:o + B])
        o += B
    assert o == N == bank.N
    rep = bank.report(ks=(1, 5))
    raw = big.cpu().numpy()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + nbytes:] == FILL).all(), "a sentinel around the bank was overwritten"
    body = raw[GUARD:GUARD + nbytes]
    if capacity > N:  # rows nobody appended are never written
        assert (body[bank._labels_at + 4 * N:bank._labels_at + 4 * capacity] == FILL).all()
        pr = body[bank._probs_at:].reshape(S * n, 4 * capacity)
        assert (pr[:, 4 * N:] == FILL).all()
    labs, probs = bank.scores()
    return bank, rep, labs, probs, body.copy()


def check(logit_sets, labels, n, rep, labs, probs):
    S, N = len(logit_sets), len(labels)
    ref = er.restate(logit_sets, labels, n)
    # integers: exactly
    assert rep["N"] == N and rep["skipped"] == ref["skipped"] and rep["nonfinite"] == list(ref["nonfinite"])
    np.testing.assert_array_equal(labs, ref["labels"])
    np.testing.assert_array_equal(rep["num"], ref["num"])
    np.testing.assert_array_equal(rep["rank_hist"], ref["rank_hist"])
    np.testing.assert_array_equal(rep["confusion"], ref["confusion"])
    for k in (1, 5):
        want = er.topk(ref["rank_hist"], k)
        for s in range(S):
            assert (np.isnan(rep["topk"][k][s]) if want[s] is None else Fraction(rep["topk"][k][s]) == Fraction(float(want[s])))
    # stored probabilities: inside the restatement's bound, NaN exactly where a row is left out
    assert probs.dtype == np.float32 and probs.shape == (S, n, N)
    out = np.isnan(ref["probs"])
    np.testing.assert_array_equal(np.isnan(probs), out)
    frac = er.excess(probs[~out], ref["probs"][~out], ref["bound"][~out]) if (~out).any() else 0.0
    WORST["probs"] = max(WORST["probs"], frac)
    print(f"evalbank probs: N {N} n {n} sets {S}: worst |p - ref| / bound = {frac:.4f} (all cases so far {WORST['probs']:.4f})")
    assert frac <= 1.0
    # average precision: against the exact value from the probabilities the kernel stored
    for s in range(S):
        exact, npos = er.ap_exact(probs[s], labs)
        bound = er.ap_bound(npos)
        kept = []
        for c in range(n):
            got = float(rep["ap"][s, c])
            if exact[c] is None:
                assert np.isnan(got), (s, c, got)
                continue
            kept.append(c)
            err = abs(Fraction(got) - exact[c])
            assert err <= Fraction(float(bound[c])), (s, c, got, float(exact[c]), float(err), bound[c])
        got = float(rep["mAP"][s])
        if not kept:
            assert np.isnan(got)
            continue
        mean = sum(exact[c] for c in kept) / len(kept)
        assert abs(Fraction(got) - mean) <= Fraction(float(bound[kept].max() + (n + 2) * er.U64)), (s, got, float(mean))
    return ref


def case(kind, N, n, S, seed=0):
    return [er.make_logits(kind, N, n, seed + s) for s in range(S)], er.make_labels(N, n, seed)


SHAPES = [(N, n, 3 if (i + j) % 2 == 0 else 1, er.SCORE_KINDS[(i + 2 * j) % 4]) for i, N in enumerate(NS) for j, n in enumerate(CLASSES)]


@pytest.mark.parametrize("N,n,S,kind", SHAPES)
def test_shapes(N, n, S, kind):
    sets, lab = case(kind, N, n, S)
    bank, rep, labs, probs, _ = run_bank(sets, lab, n)
    check(sets, lab, n, rep, labs, probs)
    again = bank.report(ks=(1, 5))  # a second call of the AP kernel: identical bytes
    assert again["ap"].tobytes() == rep["ap"].tobytes() and again["mAP"].tobytes() == rep["mAP"].tobytes()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind", er.SCORE_KINDS)
def test_score_kinds(kind, S):
    """every kind of score at one shape with several positives per class and more than one block of them (257 > 256)"""
    sets, lab = case(kind, 257, 6, S, seed=3)
    _, rep, labs, probs, _ = run_bank(sets, lab, 6)
    check(sets, lab, 6, rep, labs, probs)
    if kind == "spread":
        assert (probs < 2.0 ** -126).any(), "the spread case is meant to store subnormal or zero probabilities"


def test_appends_inside_a_tile_and_at_capacity():
    """5 + 64 + 3 rows: offsets that fall inside a tile; the last append ends exactly at the capacity.  The same rows in a
    larger bank: the rows beyond N keep the sentinel."""
    sets, lab = case("halves", 72, 6, 3, seed=5)
    for cap in (72, 100):
        _, rep, labs, probs, _ = run_bank(sets, lab, 6, capacity=cap, chunks=[5, 64, 3])
        check(sets, lab, 6, rep, labs, probs)
    one, _, _, _, body = run_bank(sets, lab, 6, capacity=72)
    _, _, _, _, body3 = run_bank(sets, lab, 6, capacity=72, chunks=[5, 64, 3])
    assert body.tobytes() == body3.tobytes(), "the appends' boundaries show in the bank"
    with pytest.raises(L.GdlError, match="do not fit"):
        one.append(*(dev(s[:1]) for s in sets), torch.from_numpy(lab[:1]).to(DEV))


def test_empty_class_and_one_class_holding_every_sample():
    sets, lab = case("random", 300, 6, 3, seed=7)
    lab[lab == 2] = 4  # class 2 has no positive: NaN, left out of the mAP
    _, rep, labs, probs, _ = run_bank(sets, lab, 6)
    check(sets, lab, 6, rep, labs, probs)
    assert np.isnan(rep["ap"][:, 2]).all() and not np.isnan(rep["mAP"]).any()
    assert np.isnan(rep["per_class_acc"][:, 2]).all()
    lab[:] = 3  # one class holds every sample (more than one pass of 256 positives): its AP is 1, every other NaN
    _, rep, labs, probs, _ = run_bank(sets, lab, 6)
    check(sets, lab, 6, rep, labs, probs)
    assert (rep["ap"][:, 3] == 1.0).all() and (rep["mAP"] == 1.0).all()


def test_bad_labels_and_nonfinite_logits():
    N, n = 130, 6
    sets, lab = case("random", N, n, 3, seed=9)
    for i, v in ((3, -1), (64, n), (65, 2 ** 31 + 1), (129, 2 ** 32 + 1)):
        lab[i] = v
    sets[1][10, 2] = np.nan       # a NaN logit in the audio set only
    sets[2][70, 5] = np.inf       # an inf logit in the visual set only
    sets[2][71, 0] = -np.inf
    sets[0][3, 1] = np.nan        # in a skipped row: counted as skipped, not as non-finite
    _, rep, labs, probs, _ = run_bank(sets, lab, n)
    ref = check(sets, lab, n, rep, labs, probs)
    assert rep["skipped"] == 4 and rep["nonfinite"] == [0, 1, 2] and ref["skipped"] == 4
    assert (labs[[3, 64, 65, 129]] == -1).all() and rep["num"].sum() == N - 4
    assert rep["confusion"][0].sum() == N - 4 and rep["confusion"][1].sum() == N - 5 and rep["confusion"][2].sum() == N - 6
    assert np.isnan(probs[1][:, 10]).all() and not np.isnan(probs[0][:, 10]).any()


def test_golden_sklearn_values():
    g = np.load(GOLDEN)
    for name in ("a", "b", "c"):
        lg, lab, want = g[name + ".logits"], g[name + ".labels"], g[name + ".ap"]
        n = lg.shape[1]
        _, rep, labs, probs, _ = run_bank([lg], lab, n)
        check([lg], lab, n, rep, labs, probs)
        npos = np.bincount(lab, minlength=n)
        for c in range(n):
            assert abs(rep["ap"][0, c] - want[c]) <= er.ap_bound(npos[c]), (name, c, rep["ap"][0, c], want[c])
        assert abs(rep["mAP"][0] - want.mean()) <= er.ap_bound(npos).max() + (n + 2) * er.U64


def test_two_runs_give_identical_bytes():
    sets, lab = case("halves", 1000, 65, 3, seed=11)
    lab[17] = -5
    sets[1][40, 0] = np.nan
    a = run_bank(sets, lab, 65, capacity=1024, chunks=[64] * 15 + [40])[4]
    b = run_bank(sets, lab, 65, capacity=1024, chunks=[64] * 15 + [40])[4]
    assert a.tobytes() == b.tobytes()


def test_reset_starts_a_new_report():
    sets, lab = case("random", 65, 6, 1, seed=13)
    bank, rep, _, _, _ = run_bank(sets, lab, 6, capacity=80)
    bank.reset()
    assert bank.N == 0
    sets2, lab2 = case("halves", 40, 6, 1, seed=14)
    bank.append(dev(sets2[0]), None, None, torch.from_numpy(lab2).to(DEV))
    rep2 = bank.report(ks=(1, 5))
    labs, probs = bank.scores()
    check(sets2, lab2, 6, rep2, labs, probs)
    assert rep2["N"] == 40 and rep["N"] == 65


def test_python_refusals_before_any_launch():
    import gdl

    bank = gdl.ScoreBank(6, 8, 3, DEV)
    o, lab = torch.zeros((4, 6), device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    for args, word in (((o, None, None, lab), "logit set"), ((o, o, o.double(), lab), "float32"),
                       ((o, o, torch.zeros((4, 7), device=DEV), lab), "float32"), ((o, o, o, lab.int()), "int64"),
                       ((o, o, o, lab[:3]), "int64"), ((o, o, o, lab.cpu()), "a tensor on")):
        with pytest.raises(L.GdlError, match=word):
            bank.append(*args)
    for n, S, rows, word in ((7, 3, 4, "n_classes"), (6, 1, 4, "sets"), (6, 3, 9, "do not fit")):
        with pytest.raises(L.GdlError, match=word):
            bank.check(n, S, DEV, rows)
    with pytest.raises(L.GdlError, match="is on cuda:0, the logits on cuda:1"):
        bank.check(6, 3, "cuda:1", 4)
    assert bank.N == 0 and int(bank.buf[:bank._reset_bytes].sum()) == 0
    for bad in ((0, 8, 3), (513, 8, 3), (6, 0, 3), (6, 8, 2)):
        with pytest.raises(L.GdlError):
            gdl.ScoreBank(*bad, DEV)
    with pytest.raises(L.GdlError, match="at least 1"):
        bank.report(ks=(0,))


# ------------------------------------------------------------------ the runners, at the tiny fixture shapes
TINY = dict(dataset="CREMAD", n_classes=6, spec_hw=[65, 47], frames=2, image_hw=[64, 64], batch=4, seed=0, lr=2e-3, alpha=2.5)
_STATE = {}


def _state():
    if not _STATE:
        P, Bf = fx.model_state(6, "concat_dgl")
        _STATE.update({k: torch.from_numpy(np.array(v)) for k, v in {**P, **Bf}.items()})
    return _STATE


def _batch(st):
    spec, image, label = fx.make_batch(TINY["seed"] + st, TINY["batch"], TINY["spec_hw"], TINY["frames"], TINY["image_hw"], 6)
    return dev(spec), dev(image), torch.from_numpy(label).to(DEV)


def _model(modality="full"):
    from models.basic_model import AVClassifier_DGL

    model = AVClassifier_DGL(argparse.Namespace(fusion_method="concat", dataset="CREMAD", modality=modality, batch_size=4))
    if modality == "full":
        model.load_state_dict(_state(), strict=True)
    else:
        keep = ("fusion_module.", modality + "_net.")
        st = {k: v for k, v in _state().items() if k.startswith(keep)}
        st.update({k: torch.from_numpy(np.array(v)) for k, v in
                   fx.make_state({modality + "_classifier.weight": (6, 512), modality + "_classifier.bias": (6,)}).items()})
        model.load_state_dict(st, strict=True)
    model = model.to(DEV)
    for net in ("audio_net", "visual_net"):
        if getattr(model, net, None) is not None:
            getattr(model, net).gdl_dtype = "f32"
    return model.train()


def _cross_check(rep, counts, acc, S):
    """the report against valid()'s own counters: rows [num, acc, acc_a, acc_v] per class"""
    assert rep["skipped"] == 0 and rep["nonfinite"] == [0] * S
    np.testing.assert_array_equal(rep["num"], counts[0])
    for s in range(S):
        np.testing.assert_array_equal(rep["confusion"][s].sum(axis=1), counts[0])
        np.testing.assert_array_equal(rep["confusion"][s].diagonal(), counts[s + 1])
        assert rep["topk"][1][s] == acc[s]
        assert rep["topk"][6][s] == 1.0


@pytest.mark.parametrize("mode", ["dgl", "joint"])
def test_trainer_valid_with_a_bank(mode):
    import gdl
    from gdl.trainer import DGLTrainer

    S = 3 if mode == "dgl" else 1
    batches = [_batch(1000), _batch(1001), _batch(1002)]
    step = _batch(0)
    runs = []
    for with_bank in (False, True):
        tr = DGLTrainer(_model(), lr=TINY["lr"], alpha=TINY["alpha"], mode=mode)
        tr.step(*step)
        bank = gdl.ScoreBank(6, 12, S, DEV) if with_bank else None
        acc = tr.valid(batches, bank=bank) if with_bank else tr.valid(batches)
        counts = tr.valid_counts.copy()
        tr.step(*step)
        r = tr.read()
        runs.append((acc, counts, r, tr.params.clone(), bank))
    (acc0, c0, r0, p0, _), (acc1, c1, r1, p1, bank) = runs
    assert acc0 == acc1 and np.array_equal(c0, c1)
    assert torch.equal(p0, p1) and r0["out"].tobytes() == r1["out"].tobytes() and r0["loss_f"] == r1["loss_f"]
    rep = bank.report(ks=(1, 6))
    assert rep["N"] == 12
    _cross_check(rep, c1, acc1, S)
    # refused before the first launch: nothing appended, the counters untouched
    tr = DGLTrainer(_model(), lr=TINY["lr"], alpha=TINY["alpha"], mode=mode)
    for bad, word in ((gdl.ScoreBank(6, 11, S, DEV), "do not fit"), (gdl.ScoreBank(7, 12, S, DEV), "n_classes"),
                      (gdl.ScoreBank(6, 12, 4 - S, DEV), "sets")):
        with pytest.raises(L.GdlError, match=word):
            tr.valid(batches, bank=bad)
        assert bad.N == 0 and int(bad.buf[:bad._reset_bytes].sum()) == 0


@pytest.mark.parametrize("modality", ["audio", "visual"])
def test_unimodal_valid_with_a_bank(modality):
    import gdl
    from gdl.unimodal import UnimodalTrainer

    batches = [_batch(1000), _batch(1001)]
    tr = UnimodalTrainer(_model(modality), lr=TINY["lr"])
    acc0 = tr.valid(batches)
    c0 = tr.valid_counts.copy()
    bank = gdl.ScoreBank(6, 8, 1, DEV)
    acc1 = tr.valid(batches, bank=bank)
    assert acc0 == acc1 and np.array_equal(c0, tr.valid_counts)
    _cross_check(bank.report(ks=(1, 6)), tr.valid_counts, acc1, 1)
    with pytest.raises(L.GdlError, match="sets"):
        tr.valid(batches, bank=gdl.ScoreBank(6, 8, 3, DEV))
    with pytest.raises(L.GdlError, match="do not fit"):
        tr.valid(batches, bank=bank)  # full


def test_linear_probe_score_with_a_bank():
    import gdl
    import probe_ref as R

    bank_np, labels, W, b, _ = R.synthetic_case(300, 64, 34)
    feats = gdl.FeatureBank(dev(bank_np), torch.from_numpy(labels).to(DEV))
    probe = gdl.LinearProbe(34, DEV)
    probe.load_state_dict(dict(weight=torch.from_numpy(W), bias=torch.from_numpy(b), momentum_weight=torch.zeros(34, 512),
                               momentum_bias=torch.zeros(34), epoch=0))
    acc0, counts0 = probe.score(feats, chunk=128)
    scores = gdl.ScoreBank(34, 300, 1, DEV)
    acc1, counts1 = probe.score(feats, chunk=128, scores=scores)  # 128 + 128 + 44: a ragged last chunk
    assert acc0 == acc1 and np.array_equal(counts0, counts1)
    rep = scores.report(ks=(1, 5, 34))
    assert rep["N"] == 300
    np.testing.assert_array_equal(rep["confusion"][0].sum(axis=1), counts1[0])
    np.testing.assert_array_equal(rep["confusion"][0].diagonal(), counts1[1])
    assert rep["topk"][1][0] == acc1 and rep["topk"][1][0] <= rep["topk"][5][0] <= rep["topk"][34][0] == 1.0
    out = torch.empty((300, 34), device=DEV)
    L.call("gdl_head_cls_fwd", L.ptr(feats.features), L.ptr(probe.weight), L.ptr(probe.bias), L.ptr(out), 300, 34, 512, L.cur_stream())
    labs, probs = scores.scores()
    check([out.cpu().numpy()], labels, 34, rep, labs, probs)
    with pytest.raises(L.GdlError, match="do not fit"):
        probe.score(feats, scores=gdl.ScoreBank(34, 299, 1, DEV))
